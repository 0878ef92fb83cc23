"""Deterministic scene and state generator for the shading fuzz tests (tests/test_shading_fuzz_host.py on the oracle alone,
tests/test_gpu_shading_fuzz.py device against oracle). Everything is drawn from numpy.random.default_rng(seed) and handed over
through the calls Device and Oracle share (initTexture, setFlattenPolicy, setState, initCameras, initLights, initMaterials,
addGeometry, addInstance), so one Scene feeds both. Geometry comes from the library's own mesh generators at low tessellation.

Feature switches of make_scene choose the build of the shade kernel a pass launches (shade_kernels.hip launchShade):
  miss 0 / 1 / 2      black, constant white, spherical environment (procedural.environment_hdr, rotated)      -> ENV
  tex                 albedo texture on the floor and on non-Lambert materials                                -> TEX
  full                cutout opacity on a glass material and a geometry shared by many instances (two-level)  -> not SLIM
                      (slim: every instance flattened, no cutout - a slim scene cannot hold a cutout material)
  band                bytes of the instance + material + light tables: "small" <= 8 KiB (fits beside the sort exchange buffer),
                      "mid" <= 20 KiB (fits the plain builds' LDS budget), "large" above                      -> LDS_TABLES, SORT
"""
import math

import numpy as np

import tweeker_raytracer_amd as twk
from procedural import albedo_checker, cutout_slots, environment_hdr

WIDTH, HEIGHT = 61, 37  # neither a multiple of the 8 x 8 tile nor of 256 paths

# Bytes of a record in the tables the shade kernel stages in LDS, and the two budgets launchShade compares their sum with. The host
# test checks these against the product's sources (static_asserts of device_handle.h, #defines of shade_kernels.hip).
INSTANCE_BYTES, MATERIAL_BYTES, LIGHT_BYTES = 128, 64, 80
SORT_TABLE_BYTES, TABLE_BYTES = 8192, 20480
BANDS = ("small", "mid", "large")
CONFETTI = {"small": 0, "mid": 40, "large": 130}  # extra two-triangle instances per band

BSDF_NAMES = ("diffuse", "mirror", "glass", "ggx", "ggx_glass")
ABSORPTION_SCALES = (0.0, 0.5, 20.0, 1000.0)
NESTED_RADII = (1.0, 0.86, 0.72, 0.58, 0.44, 0.30)  # six deep: deeper than the four entries of the volume stack

M_LIGHT, M_FLOOR, M_FUZZ0 = 0, 1, 2  # material indices: the lights' black material, the floor, then the 20 drawn ones
NUM_FUZZ = 20                        # 5 BSDFs x thin-walled 0 / 1 x 2 draws


def material(bsdf=0, albedo=(0.7, 0.7, 0.7), absorptionColor=(1.0, 1.0, 1.0), absorptionScale=0.0, ior=1.5, thinwalled=0,
             albedoTexture=0, cutoutTexture=0, roughness=(0.1, 0.1)):
    m = twk.MaterialGUI()
    m.indexBSDF = int(bsdf)
    for k in range(3):
        m.albedo[k] = float(albedo[k])
        m.absorptionColor[k] = float(absorptionColor[k])
    m.absorptionScale, m.ior, m.thinwalled = float(absorptionScale), float(ior), int(thinwalled)
    m.useAlbedoTexture, m.useCutoutTexture = int(albedoTexture), int(cutoutTexture)
    m.roughness[0], m.roughness[1] = float(roughness[0]), float(roughness[1])
    return m


def environment_light():
    l = twk.LightDefinition()
    l.type = 0
    l.vecU[0], l.vecV[1], l.normal[2] = 1.0, 1.0, 1.0
    l.area = np.float32(4.0) * np.float32(math.pi)
    l.emission[0] = l.emission[1] = l.emission[2] = 1.0
    return l


def parallelogram_light(position, size, emission):
    """A square light of edge `size` in the xz plane with its corner at `position`, lit side down (normal = cross(vecU, vecV))."""
    l = twk.LightDefinition()
    l.type = 1
    for k in range(3):
        l.position[k] = float(position[k])
        l.emission[k] = float(emission[k])
    l.vecU[0], l.vecV[2] = float(size), float(size)
    l.normal[1] = -1.0
    l.area = float(np.float32(size) * np.float32(size))
    return l


def transform(scale=1.0, translate=(0.0, 0.0, 0.0), angle_x=0.0):
    """Row-major 3 x 4: uniform scale, rotation about x, translation."""
    c, s = math.cos(angle_x), math.sin(angle_x)
    r = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64) * scale
    return np.concatenate([r, np.asarray(translate, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(12)


class Scene:
    def __init__(self):
        self.miss, self.tex, self.full, self.band, self.seed = 1, False, False, "small", 0
        self.textures, self.lights, self.materials, self.geometries, self.instances = [], [], [], [], []
        self.flatten = (4, 2)
        self.camera = None
        self.env_rotation = 0.0

    @property
    def features(self):
        return (self.miss, self.tex, "full" if self.full else "slim", self.band)

    @property
    def table_bytes(self):
        return len(self.instances) * INSTANCE_BYTES + len(self.materials) * MATERIAL_BYTES + len(self.lights) * LIGHT_BYTES

    @property
    def predicted_band(self):
        b = self.table_bytes
        return "small" if b <= SORT_TABLE_BYTES else ("mid" if b <= TABLE_BYTES else "large")

    @property
    def predicted_layout(self):
        """slim: every instance flattened (at most flatten[0] triangles, or a geometry of at most flatten[1] instances) and no cutout."""
        refs = {}
        for g, _, _, _ in self.instances:
            refs[g] = refs.get(g, 0) + 1
        flat = all(len(self.geometries[g][1]) // 3 <= self.flatten[0] or refs[g] <= self.flatten[1] for g in refs)
        cutout = any(m.useCutoutTexture for m in self.materials)
        return "slim" if flat and not cutout else "full"

    def arrays(self):
        """Everything the scene hands over, as bytes: what 'the same seed gives byte-equal arrays' compares."""
        out = [np.asarray(t, np.float32).tobytes() for _, t in self.textures]
        out += [bytes(l) for l in self.lights] + [bytes(m) for m in self.materials] + [bytes(self.camera)]
        out += [a.tobytes() + i.tobytes() for a, i in self.geometries]
        out += [np.asarray([g, m, l], np.int32).tobytes() + np.asarray(t, np.float32).tobytes() for g, t, m, l in self.instances]
        return b"".join(out)


def _log_uniform(rng, lo, hi):
    return float(np.float32(math.exp(rng.uniform(math.log(lo), math.log(hi)))))


def _fuzz_materials(rng, tex, range_ends):
    """20 materials: every BSDF, thin-walled 0 and 1, two draws each. Roughness log-uniform in [0.001, 1] per axis, with the exact
    value 1 and a strongly anisotropic pair forced in; ior in [0.5, 3] with exactly 1.0 forced in; absorption scales cycle through
    ABSORPTION_SCALES. range_ends: roughness 0 on one or both axes and ior at the ends of the GUI's range (Application.cpp:956,965)."""
    mats = []
    for draw in range(2):
        for bsdf in range(5):
            for thin in range(2):
                k = len(mats)
                rough = [_log_uniform(rng, 0.001, 1.0), _log_uniform(rng, 0.001, 1.0)]
                ior = float(np.float32(rng.uniform(0.5, 3.0)))
                if draw == 0 and bsdf >= 3:
                    rough = ([1.0, 1.0], [0.001, 1.0])[thin]        # the exact upper end; 1000 : 1 anisotropy
                if draw == 1 and bsdf in (2, 4) and thin == 0:
                    ior = 1.0
                if range_ends:
                    rough = ([0.0, 0.0], [0.0, rough[1]], [rough[0], 0.0], rough)[k % 4]
                    ior = (0.0, 10.0, ior)[k % 3]
                mats.append(material(bsdf, albedo=rng.uniform(0.2, 1.0, 3), absorptionColor=rng.uniform(0.05, 1.0, 3),
                                     absorptionScale=ABSORPTION_SCALES[(k + draw) % 4], ior=ior, thinwalled=thin,
                                     albedoTexture=int(tex and bsdf != 0 and draw == 1), roughness=rough))
    return mats


def make_scene(seed, miss=1, tex=False, full=False, band="small", range_ends=False):
    rng = np.random.default_rng(seed)
    s = Scene()
    s.seed, s.miss, s.tex, s.full, s.band = seed, miss, bool(tex), bool(full), band
    s.flatten = (4, 2) if full else (1 << 20, 1 << 20)
    s.camera = twk.camera_frustum((0.0, 0.0, 0.0), 0.75, 0.5, 50.0, 7.0, WIDTH / HEIGHT)
    if tex:
        s.textures.append((0, albedo_checker()))
    if full:
        s.textures.append((1, cutout_slots()))
    if miss == 2:
        s.textures.append((2, environment_hdr(64, 32)))
        s.env_rotation = float(np.float32(rng.uniform(0.1, 0.9)))

    # lights: the environment is light 0 when there is one; three parallelograms of different size and emission
    if miss != 0:
        s.lights.append(environment_light())
    quads = (((-2.2, 3.0, -1.0), 1.5, (6.0, 6.0, 6.0)), ((0.8, 2.6, 0.4), 0.8, (15.0, 12.0, 9.0)), ((-0.3, 3.4, -2.0), 0.4, (40.0, 30.0, 50.0)))
    first_quad = len(s.lights)
    for pos, size, emission in quads:
        s.lights.append(parallelogram_light(pos, size, emission))

    # materials
    s.materials.append(material(1, albedo=(0.0, 0.0, 0.0), thinwalled=1))                      # M_LIGHT
    s.materials.append(material(0, albedo=(0.8, 0.8, 0.8), albedoTexture=int(tex)))             # M_FLOOR
    s.materials += _fuzz_materials(rng, tex, range_ends)
    m_nested = len(s.materials)
    for k in range(3):  # the nested spheres' media: plain glass, different ior and absorption, never thin-walled
        s.materials.append(material(2, albedo=(1.0, 1.0, 1.0), absorptionColor=rng.uniform(0.3, 1.0, 3), absorptionScale=(0.5, 0.0, 20.0)[k],
                                    ior=(1.5, 1.2, 1.8)[k]))
    m_bowl = len(s.materials)
    s.materials.append(material(4, albedo=(0.9, 0.95, 1.0), ior=1.4, roughness=(0.05, 0.3), albedoTexture=int(tex)))
    if full:
        s.materials[M_FUZZ0 + 2 * 2].useCutoutTexture = 1  # first draw, BSDF 2 (glass), not thin-walled

    def add(geometry, t, m, light=-1):
        s.instances.append((geometry, t, m, light))

    def geometry(mesh):
        s.geometries.append((np.ascontiguousarray(mesh[0], np.float32), np.ascontiguousarray(mesh[1], np.uint32)))
        return len(s.geometries) - 1

    g_plane = geometry(twk.mesh_plane(1, 1, 1))
    add(g_plane, transform(5.0, (0.0, -1.2, 0.0)), M_FLOOR)
    for k, (pos, size, _) in enumerate(quads):
        l = s.lights[first_quad + k]
        g = geometry(twk.mesh_parallelogram(list(l.position), list(l.vecU), list(l.vecV), list(l.normal)))
        add(g, transform(), M_LIGHT, first_quad + k)
    for k, r in enumerate(NESTED_RADII):  # one geometry each: referenced once, so flattened under either policy
        add(geometry(twk.mesh_sphere(12, 6, r, math.pi)), transform(1.0, (-1.6, 0.0, 0.0)), m_nested + k % 3)
    add(geometry(twk.mesh_sphere(12, 4, 0.8, 0.5 * math.pi)), transform(1.0, (1.8, -0.3, -0.6), angle_x=float(rng.uniform(-0.6, 0.6))), m_bowl)  # open half sphere
    g_ball = geometry(twk.mesh_sphere(10, 5, 1.0, math.pi))  # shared by 20 instances: two-level under the default policy
    for k in range(NUM_FUZZ):
        i, j = k % 5, k // 5
        jitter = rng.uniform(-0.05, 0.05, 3)
        add(g_ball, transform(0.27, (-1.0 + 0.7 * i + jitter[0], -0.9 + 0.6 * j + jitter[1], 1.7 - 0.35 * j + jitter[2]), angle_x=float(rng.uniform(0, math.pi))),
            M_FUZZ0 + k)
    for k in range(CONFETTI[band]):  # two triangles each: flattened under either policy; they fill the tables
        add(g_plane, transform(float(rng.uniform(0.05, 0.15)), rng.uniform((-2.8, -1.0, -2.8), (2.8, 2.2, 0.8)), angle_x=float(rng.uniform(0, math.pi))),
            M_FUZZ0 + int(rng.integers(NUM_FUZZ)))
    return s


def default_state(scene, pathLengths=(2, 6), samplesSqrt=1, lensShader=0, epsilonFactor=500.0):
    st = twk.DeviceState()
    st.resolution[0], st.resolution[1] = WIDTH, HEIGHT
    st.tileSize[0], st.tileSize[1] = 8, 8
    st.pathLengths[0], st.pathLengths[1] = pathLengths
    st.distribution, st.samplesSqrt, st.lensShader = 0, int(samplesSqrt), int(lensShader)
    st.epsilonFactor, st.envRotation, st.clockFactor = float(epsilonFactor), float(scene.env_rotation), 1000.0
    return st


PATH_MIN, PATH_MAX = (0, 1, 2, 5), (1, 2, 6, 16)
EPSILON_FACTORS = (50.0, 500.0, 1000.0, 5000.0)
SWEEP_SEEDS = tuple(range(1000, 1024))


def draw_case(seed):
    """One state-sweep case: the scene's feature switches and the whole pass state, all from the seed."""
    rng = np.random.default_rng([seed, 0x57A7E])
    pick = lambda values: values[int(rng.integers(len(values)))]
    case = {
        "seed": seed,
        "miss": pick((0, 1, 2)), "tex": pick((False, True)), "full": pick((False, True)),
        "pathLengths": (pick(PATH_MIN), pick(PATH_MAX)),
        "lensShader": pick((0, 1, 2)), "samplesSqrt": pick((1, 2, 3)), "epsilonFactor": pick(EPSILON_FACTORS),
        "variant": pick((0, 1)), "nee": pick((True, False)), "half": pick((False, True)), "batchAll": pick((False, True)),
    }
    return case


def case_scene(case):
    return make_scene(case["seed"], case["miss"], case["tex"], case["full"], "mid")


def case_state(case, scene):
    return default_state(scene, case["pathLengths"], case["samplesSqrt"], case["lensShader"], case["epsilonFactor"])


def feed(target, scene, state):
    """The shared call sequence: target is a Device or an Oracle."""
    for slot, image in scene.textures:
        target.initTexture(slot, image)
    target.setFlattenPolicy(*scene.flatten)
    target.setState(state)
    target.initCameras([scene.camera])
    target.initLights(scene.lights)
    target.initMaterials(scene.materials)
    for attributes, indices in scene.geometries:
        target.addGeometry(attributes, indices)
    for g, t, m, l in scene.instances:
        target.addInstance(g, t, m, l)
    target.build()


def render_oracle(orc, scene, state, iterations, variant=0, nee=True, half=False, aov=False):
    """(oracle, image, [albedo, normal] or None) after `iterations` iterations."""
    ref = orc.Oracle(miss=scene.miss, nee=nee)
    feed(ref, scene, state)
    ref.setShaderVariant(variant)
    ref.enableAov(aov)
    ref.setOutputHalf(half)
    for it in range(iterations):
        ref.render(it)
    return ref, ref.getOutputBufferHost().copy(), ([ref.readAov(0).copy(), ref.readAov(1).copy()] if aov else None)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mismatch(got, want, nan_positions_only=False):
    """None when the images agree bit for bit; otherwise 'N pixels differ, first at x=.., y=..: got .. want ..' - the pixel goes
    straight into tools/debug_pixel_mismatch.py or Oracle.debugPath. nan_positions_only: where `want` is NaN, `got` must be NaN
    (payload and sign free); every other value is compared bit for bit, infinities included."""
    differ = bits(got) != bits(want)
    if nan_positions_only:
        differ = np.where(np.isnan(want), ~np.isnan(got), differ)
    pixels = differ.any(axis=2)
    if not pixels.any():
        return None
    y, x = (int(v) for v in np.argwhere(pixels)[0])
    return f"{int(pixels.sum())} pixels differ, first at x={x}, y={y}: got {got[y, x].tolist()} want {want[y, x].tolist()}"


# ---- analytic anchors ---------------------------------------------------------------------------------------------------
ANCHOR_DEPTH = 12


def invisible_glass_scene():
    """White constant environment, objects of ior 1.0, albedo 1, absorption scale 0: plain and rough glass, thin-walled and not.
    Light passes straight through with throughput exactly 1, so every pixel is exactly 1.0."""
    s = Scene()
    s.miss = 1
    s.camera = twk.camera_frustum((0.0, 0.0, 0.0), 0.75, 0.5, 50.0, 7.0, WIDTH / HEIGHT)
    s.lights = [environment_light()]
    for bsdf in (2, 4):
        for thin in (0, 1):
            s.materials.append(material(bsdf, albedo=(1.0, 1.0, 1.0), absorptionColor=(0.3, 0.5, 0.7), absorptionScale=0.0, ior=1.0, thinwalled=thin,
                                        roughness=(0.2, 0.6)))
    s.geometries.append(tuple(np.ascontiguousarray(a) for a in twk.mesh_sphere(16, 8, 1.0, math.pi)))
    s.geometries.append(tuple(np.ascontiguousarray(a) for a in twk.mesh_box()))
    for k, pos in enumerate(((-1.5, 0.8, 0.0), (1.5, 0.8, 0.0), (-1.5, -0.9, 0.5), (1.5, -0.9, 0.5))):
        s.instances.append((k % 2, transform(0.8, pos), k, -1))
    return s, default_state(s, (ANCHOR_DEPTH, ANCHOR_DEPTH))


SLAB_HALF_THICKNESS = 0.25
SLAB_COLOR, SLAB_SCALE = (0.8, 0.5, 0.25), 1.5
SLAB_FOV, SLAB_DISTANCE = 40.0, 6.0


def slab_scene():
    """A box slab (x, y in [-3, 3], z in [-0.25, 0.25]) of ior 1.0 plain glass with absorption, in the white constant environment,
    seen by a pinhole camera on the +z axis looking down -z: every primary ray crosses both faces and nothing else."""
    s = Scene()
    s.miss = 1
    s.camera = twk.camera_frustum((0.0, 0.0, 0.0), 0.75, 0.5, SLAB_FOV, SLAB_DISTANCE, WIDTH / HEIGHT)
    s.lights = [environment_light()]
    s.materials.append(material(2, albedo=(1.0, 1.0, 1.0), absorptionColor=SLAB_COLOR, absorptionScale=SLAB_SCALE, ior=1.0))
    s.geometries.append(tuple(np.ascontiguousarray(a) for a in twk.mesh_box()))  # the cube [-1, 1]^3
    s.instances.append((0, np.array([4.5, 0, 0, 0, 0, 3.0, 0, 0, 0, 0, SLAB_HALF_THICKNESS, 0], np.float32), 0, -1))
    return s, default_state(s, (ANCHOR_DEPTH, ANCHOR_DEPTH))


def slab_expected_interval(camera):
    """Per pixel and channel [lo, hi] of exp(-sigma * thickness / cos(theta)) over the pixel's footprint, in float64. sigma as
    twk_init_materials documents it (Device.cpp:1022-1050): -log(max(0.0001, colour)) * scale. theta is the angle between the
    primary ray U * ndc.x + V * ndc.y + W (ndc = (pixel + jitter) / screen * 2 - 1, jitter in [0, 1)^2) and the slab's normal z."""
    U, V, W = (np.array(list(v), np.float64) for v in (camera.U, camera.V, camera.W))
    sigma = -np.log(np.maximum(0.0001, np.array(SLAB_COLOR, np.float64))) * SLAB_SCALE
    thickness = 2.0 * SLAB_HALF_THICKNESS

    def inv_cos(nx, ny):
        d = U[None, None, :] * nx[..., None] + V[None, None, :] * ny[..., None] + W[None, None, :]
        return np.sqrt((d * d).sum(-1)) / np.abs(d[..., 2])

    x0 = np.arange(WIDTH, dtype=np.float64) / WIDTH * 2 - 1
    x1 = (np.arange(WIDTH, dtype=np.float64) + 1) / WIDTH * 2 - 1
    y0 = np.arange(HEIGHT, dtype=np.float64) / HEIGHT * 2 - 1
    y1 = (np.arange(HEIGHT, dtype=np.float64) + 1) / HEIGHT * 2 - 1
    # 1 / cos grows with |ndc.x| and |ndc.y| (U, V, W orthogonal, W along the normal): its extremes over a pixel are at the
    # footprint's points of least and greatest |ndc|
    near = lambda a, b: np.where((a <= 0) & (b >= 0), 0.0, np.minimum(np.abs(a), np.abs(b)))
    far = lambda a, b: np.maximum(np.abs(a), np.abs(b))
    nx_lo, ny_lo = np.meshgrid(near(x0, x1), near(y0, y1))
    nx_hi, ny_hi = np.meshgrid(far(x0, x1), far(y0, y1))
    hi = np.exp(-sigma[None, None, :] * thickness * inv_cos(nx_lo, ny_lo)[..., None])
    lo = np.exp(-sigma[None, None, :] * thickness * inv_cos(nx_hi, ny_hi)[..., None])
    return lo, hi


# Beer-Lambert tolerance, absolute, derived (u = 2^-24, the unit roundoff of fp32; nothing here was read off a run):
#   the exponent E = sigma * d with E <= -ln(0.25) * 1.5 * 0.5 * 1.25 = 1.3 here (1 / cos <= 1.25 inside the frustum);
#   sigma: logf (<= 2u relative), the multiply by the scale (u): 3u;
#   d = the back face's hit distance from the front face's hit point. The front hit point o + t * dir carries t's error (a
#     triangle test: <= 8 roundings, 8u of t <= 7.5) and its own multiply-add (2u of coordinates <= 6.5): <= 73u absolute; the
#     back hit distance the same test again on d ~ 0.5..0.63: 8u relative; ray direction normalisation 4u. Relative to d >= 0.5:
#     146u + 12u = 158u;
#   the product sigma * d (u) and the negation: E's relative error <= 162u = 9.7e-6;
#   exp(-E) turns a relative error r of E into r * E * exp(-E) <= r / e absolute: 3.6e-6; the oracle's exp is within 2 ulp of the
#   correctly rounded value (tests/test_oracle_math.py), <= 2.5 ulp = 5u of a value <= 1: 3.0e-7; throughput * radiance (1.0): exact.
SLAB_TOLERANCE = 162 * 2.0 ** -24 / math.e + 5 * 2.0 ** -24

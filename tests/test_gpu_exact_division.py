"""-m gpu: the traversal kernel's short divisions (csrc/trace_device.h exactReciprocal / exactQuotients) and its single merge of a
triangle pair (trace_persistent.h). The divisions must equal the compiler's `/` in every bit: the reciprocal on all 2^32 bit
patterns, the quotients of woopSetup on 10^8 seeded pairs, on unit directions and on constructed cases (twk_debug_exact_division
compares both in one kernel); operands that leave the short sequences for the `/` fallback must be exactly the documented classes.
The pair merge is held to the single-ray traversal, pairs on and off, closest hit and any hit, coincident quads of two instances
included; images of the Cornell box and of a two-level scene are the oracle's bit for bit (the oracle divides with the host's `/`)."""
import numpy as np
import pytest

from conftest import load_app
from test_gpu_triangle_pairs import FLOOR, TILTED, _bits, _device, _oracle_image, _rays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(twk):
    d = twk.Device(ordinal=0, miss=1)
    yield d
    d.close()


# ---- reciprocal -------------------------------------------------------------------------------------------------------------
# The short path's range is 2^-126 <= |x| <= 2^126 (bits 0x00800000 .. 0x7e800000): neither x nor 1 / x is denormal.
# Everything else takes the fallback: zero and denormals below, |x| > 2^126, infinities and NaNs above.
_LO, _HI = 0x00800000, 0x7E800000
_CLASSES = [
    ("zero and denormals", 0x00000000, _LO, True),
    ("2^-126 .. 2^126", _LO, _HI + 1, False),
    ("above 2^126, infinity, NaN", _HI + 1, 0x80000000, True),
]


@pytest.mark.parametrize("sign", [0, 0x80000000])
@pytest.mark.parametrize("name,first,end,fallback", _CLASSES)
def test_reciprocal_equals_division_on_every_bit_pattern(dev, sign, name, first, end, fallback):
    """The three classes of both signs are the 2^32 patterns; a class is swept in chunks of at most 2^28."""
    chunk = 1 << 28
    for start in range(first, end, chunk):
        count = min(chunk, end - start)
        mismatches, fallbacks, offenders = dev.debugExactDivision(first=sign | start, count=count)
        print(f"{name} sign {sign >> 31} from {start:#010x}: {count} patterns, {mismatches} mismatches, {fallbacks} fallbacks")
        assert mismatches == 0, [hex(b) for b, _ in offenders]
        assert fallbacks == (count if fallback else 0), name


def test_the_classes_are_all_bit_patterns():
    assert [c[1] for c in _CLASSES] + [0x80000000] == [0] + [c[2] for c in _CLASSES]
    assert 2 * sum(c[2] - c[1] for c in _CLASSES if c[3]) == 67108862  # the patterns the probe counts outside the range


# ---- quotients --------------------------------------------------------------------------------------------------------------
def _proven(x, d):
    """trace_device.h exactQuotientsProven, for |x| <= |d|"""
    with np.errstate(invalid="ignore"):
        return (np.abs(x) >= np.float32(2.0 ** -60)) & (np.abs(d) <= np.float32(2.0 ** 60))


def _check_pairs(dev, x, d):
    x, d = np.ascontiguousarray(x, np.float32).reshape(-1), np.ascontiguousarray(d, np.float32).reshape(-1)
    finite = np.isfinite(x) & np.isfinite(d)
    assert (np.abs(x[finite]) <= np.abs(d[finite])).all()
    mismatches, fallbacks, offenders = dev.debugExactDivision(x=x, d=d)
    print(f"{x.size} pairs: {mismatches} mismatches, {fallbacks} fallbacks")
    assert mismatches == 0, [(hex(a), hex(b)) for a, b in offenders]
    assert fallbacks == int((~_proven(x, d)).sum())
    return fallbacks


def test_quotients_on_seeded_pairs(dev):
    """10^8 pairs drawn on the device: half with |d| in [0.5, 1), half with d in every binade; x up to 70 binades below d."""
    count = 100_000_000
    mismatches, fallbacks, offenders = dev.debugExactDivision(seed=25, count=count)
    print(f"{count} seeded pairs: {mismatches} mismatches, {fallbacks} fallbacks")
    assert mismatches == 0, [(hex(a), hex(b)) for a, b in offenders]
    assert 0.1 * count < fallbacks < 0.6 * count  # both the short sequence and the fallback were taken


def test_quotients_on_directions(dev):
    """Unit directions and unnormalised ones over many binades: the dominant component divides the other two, as woopSetup does."""
    rng = np.random.default_rng(25)
    v = rng.normal(size=(1 << 20, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[1::2] *= np.exp2(rng.integers(-70, 71, (v[1::2].shape[0], 1)).astype(np.float64))
    v = v.astype(np.float32)
    k = np.abs(v).argmax(axis=1)
    rows = np.arange(v.shape[0])
    d = v[rows, k]
    x = np.concatenate([v[rows, (k + 1) % 3], v[rows, (k + 2) % 3]])
    fallbacks = _check_pairs(dev, x, np.concatenate([d, d]))
    assert 0 < fallbacks < 0.2 * x.size


def test_quotients_on_constructed_cases(dev):
    rng = np.random.default_rng(26)
    xs, ds = [], []

    def add(x, d):
        x, d = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(d, np.float32))
        for sx in (1.0, -1.0):
            for sd in (1.0, -1.0):
                xs.append((x * np.float32(sx)).ravel())
                ds.append((d * np.float32(sd)).ravel())

    exponents = np.arange(1, 255, dtype=np.uint32)
    all_ones = ((exponents << 23) | 0x7FFFFF).view(np.float32)  # d with an all-ones significand, every binade
    for scale in (1.0, 0.5, 0.99999994, 2.0 ** -12, 2.0 ** -23, 2.0 ** -24, 3.0e-5, 0.7071068):
        with np.errstate(under="ignore"):
            add(all_ones * np.float32(scale), all_ones)
    add((rng.integers(0, 1 << 23, (254, 64), dtype=np.uint32) | (np.maximum(exponents, 24)[:, None] - 23 << 23)).view(np.float32), all_ones[:, None])
    some = np.exp2(rng.uniform(-100, 100, 4096)).astype(np.float32)
    add(0.0, some)                                    # x zero: the sign of the zero quotient
    add(some, some)                                   # x = +-d
    add(np.float32(1.0e-45) * rng.integers(1, 1 << 23, 4096).astype(np.float32), np.maximum(some, np.float32(1.0e-38)))  # x denormal
    add(np.minimum(some * np.float32(2.0 ** -40), some), some)  # x tiny beside d
    # the guards' own edges: x at and just below 2^-60, d at and just above 2^60
    edge_x = np.array([2.0 ** -60, np.nextafter(np.float32(2.0 ** -60), np.float32(0)), np.nextafter(np.float32(2.0 ** -60), np.float32(1))], np.float32)
    edge_d = np.array([2.0 ** 60, np.nextafter(np.float32(2.0 ** 60), np.float32(0)), np.nextafter(np.float32(2.0 ** 60), np.float32(np.inf))], np.float32)
    add(edge_x[:, None], np.array([2.0 ** -60, 1.0, 0.75, 2.0 ** 60], np.float32)[None, :] * np.float32(1.0000001))
    add(np.array([1.0, 2.0 ** -60, 2.0 ** 59], np.float32)[:, None], edge_d[None, :])
    add(some, np.inf)
    add(np.nan, some)
    x, d = np.concatenate(xs), np.concatenate(ds)
    with np.errstate(invalid="ignore"):
        swap = np.abs(x) > np.abs(d)
    x[swap], d[swap] = d[swap], x[swap]
    fallbacks = _check_pairs(dev, x, d)
    assert 0 < fallbacks < x.size


# ---- one merge per pair -------------------------------------------------------------------------------------------------------
def _pair_scenes(twk):
    plane1 = twk.mesh_plane(1, 1, 1)
    return {
        "sphere 8 4": ([twk.mesh_sphere(8, 4, 1.0, np.pi), plane1], [(0, TILTED), (1, FLOOR)]),
        "single quad": ([plane1], [(0, TILTED)]),
        # the same quad twice: every hit ties in t between the two instances, and on the diagonal between the two halves as well
        "coincident quads of two instances": ([plane1], [(0, TILTED), (0, TILTED)]),
    }


@pytest.mark.parametrize("name", ["sphere 8 4", "single quad", "coincident quads of two instances"])
def test_single_pair_merge_against_the_single_ray_traversal(twk, monkeypatch, name):
    geometries, instances = _pair_scenes(twk)[name]
    records = []
    for pairs in (True, False):
        dev = _device(twk, monkeypatch, geometries, instances, pairs)
        info = dev.buildInfo()
        assert (info["pairLeaves"] > 0) == pairs
        _, _, tris, _ = dev.readAcceleration()
        slot_primitive = tris[:, 3].view(np.int32)
        closest = _rays(tris) if not records else records[0][0]
        shadow = closest.copy()
        shadow[:, 7] = np.random.default_rng(4).uniform(0.3, 1.5, shadow.shape[0]).astype(np.float32)  # ends before, at and beyond the target
        rec, inst, occ = dev.debugTraceQueue(closest, shadow)
        q_tbg, q_ids = dev.traceRays(closest)
        _, s_ids = dev.traceRays(shadow, anyHit=True)
        dev.close()
        hit = q_ids[:, 0] >= 0
        assert 0.2 < hit.mean() < 0.999, hit.mean()
        assert np.array_equal(inst, q_ids[:, 0]), f"{name}: {(inst != q_ids[:, 0]).sum()} instances differ"
        prim = slot_primitive[rec[hit, 3].view(np.int32)]
        assert np.array_equal(prim, q_ids[hit, 1]), f"{name}: {(prim != q_ids[hit, 1]).sum()} primitives differ"
        assert np.array_equal(_bits(rec[hit, :3]), _bits(q_tbg[hit])), f"{name}: t / beta / gamma differ"
        assert np.array_equal(occ, s_ids[:, 0]), f"{name}: {(occ != s_ids[:, 0]).sum()} occlusion flags differ"
        assert 0.02 < occ.mean() < 0.98
        if len(instances) == 2 and instances[0] == instances[1]:
            assert (inst[hit] == 0).all()  # a tie in t goes to the smaller instance
        records.append((closest, _bits(rec[:, :3])[hit], inst, prim, occ))
    on, off = records
    for k in range(1, 5):
        assert np.array_equal(on[k], off[k]), f"{name}: pairs on and off differ in {('t / beta / gamma', 'instance', 'primitive', 'occlusion')[k - 1]}"


# ---- images -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system,scene,resolution", [
    ("system_rtigo3_cornell_box.txt", "scene_rtigo3_cornell_box.txt", (96, 64)),
    ("system_rtigo3_instances.txt", "scene_rtigo3_instances.txt", (48, 32)),
])
def test_images_equal_the_oracle(twk, orc, system, scene, resolution):
    iterations = 4
    app = load_app(twk, system, scene, resolution)
    cpu = _oracle_image(orc, app, scene, iterations)  # shared with tests/test_gpu_triangle_pairs.py: same frames, same iterations
    dev = twk.Device(ordinal=0, miss=app.info.miss)
    app.initDevice(dev)
    for it in range(iterations):
        dev.render(it)
    dev.synchronizeStream()
    gpu = dev.getOutputBufferHost()
    dev.close()
    mism = (_bits(gpu) != _bits(cpu)).any(axis=2).sum()
    assert mism == 0, f"{mism} of {resolution[0] * resolution[1]} pixels differ from the oracle"

/*
 * tweeker_hip.h — C ABI of the MI355X-native path-tracing hot path.
 *
 * This is the drop-in seam that stands where rtigo3 talks to libnvoptix.so.1:
 *   - the run-time loaded OptiX function table      (reference apps/rtigo3/src/Device.cpp:504-536)
 *   - the per-GPU `Device` object wrapping it       (reference apps/rtigo3/inc/Device.h:292-404)
 * Everything is plain C: opaque handle, POD structs, pointers and sizes. No C++/torch types.
 * Every call returns 0 on success or a TwkResult error code; twk_last_error() returns the text
 * (≙ OptixResult/CUresult + CheckMacros.h:38-80 which throw std::runtime_error; a C ABI never throws).
 *
 * A handle is NOT thread safe; one handle per GPU; all work of a handle is enqueued on its own
 * non-blocking HIP stream (≙ Device.cpp:255) and calls of different handles may be interleaved
 * from one host thread.
 *
 * The library never computes on the CPU: without a usable HIP device every compute entry point
 * fails with TWK_ERROR_NO_DEVICE.
 */
#ifndef TWEEKER_HIP_H
#define TWEEKER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: TwkLaunchStats grew by waveCycles[6] (twk_stats_get writes sizeof(TwkLaunchStats) bytes) and
 * twk_debug_read_acceleration hands out the 64-byte quantised wide nodes instead of 128-byte ones. */
/* 8: TwkBuildInfo grew by wide8Nodes / wide8Levels; TwkAccelerationInfo.reserved became nodeFloats — twk_debug_read_acceleration
 * hands out the compressed 8-ary nodes (20 floats each) where the persistent kernel walks those. */
/* 9: TwkLaunchStats grew by the shade kernel's per-phase tallies; twk_set_next_event_estimation, twk_set_debug_exceptions. */
#define TWK_ABI_VERSION 9

typedef enum TwkResult
{
  TWK_SUCCESS              = 0,
  TWK_ERROR_INVALID_VALUE  = 1,
  TWK_ERROR_NO_DEVICE      = 2, /* no HIP device / HIP runtime failure at create */
  TWK_ERROR_HIP            = 3, /* a HIP call failed, text in twk_last_error() */
  TWK_ERROR_INVALID_STATE  = 4, /* call order violated (e.g. launch before build) */
  TWK_ERROR_OUT_OF_MEMORY  = 5,
  TWK_ERROR_IO             = 6, /* scene/system description file problems */
  TWK_ERROR_PARSE          = 7
} TwkResult;

/* ---- POD layouts shared with the reference (sizes asserted in the implementation) ---------- */

/* ≙ CameraDefinition, reference shaders/camera_definition.h:34-40 (48 B) */
typedef struct TwkCameraDefinition
{
  float P[3];
  float U[3];
  float V[3];
  float W[3];
} TwkCameraDefinition;

/* ≙ LightType, reference shaders/light_definition.h:34-40 */
enum { TWK_LIGHT_ENVIRONMENT = 0, TWK_LIGHT_PARALLELOGRAM = 1 };

/* ≙ LightDefinition, reference shaders/light_definition.h:42-59 (80 B) */
typedef struct TwkLightDefinition
{
  int   type;
  float position[3];
  float vecU[3];
  float vecV[3];
  float normal[3];
  float area;
  float emission[3];
  float unused0, unused1, unused2;
} TwkLightDefinition;

/* ≙ FunctionIndex, reference shaders/function_indices.h:51-60 */
enum
{
  TWK_INDEX_BRDF_DIFFUSE   = 0,
  TWK_INDEX_BRDF_SPECULAR  = 1,
  TWK_INDEX_BSDF_SPECULAR  = 2,
  TWK_INDEX_BRDF_GGX_SMITH = 3,
  TWK_INDEX_BSDF_GGX_SMITH = 4
};

/* ≙ LensShader, reference shaders/function_indices.h:42-49 */
enum { TWK_LENS_SHADER_PINHOLE = 0, TWK_LENS_SHADER_FISHEYE = 1, TWK_LENS_SHADER_SPHERE = 2 };

/* ≙ MaterialGUI without the name, reference inc/MaterialGUI.h:39-52. The device-side
 * MaterialDefinition (absorption coefficient, FLAG_THINWALLED) is derived inside
 * twk_init_materials exactly as Device::initMaterials does (Device.cpp:1022-1050). */
typedef struct TwkMaterialGUI
{
  int   indexBSDF;
  float albedo[3];
  float absorptionColor[3];
  float absorptionScale;
  float ior;
  int   thinwalled;
  int   useAlbedoTexture;
  int   useCutoutTexture;
  float roughness[2];
} TwkMaterialGUI;

/* ≙ TriangleAttributes, reference shaders/vertex_attributes.h:34-40 (48 B) */
typedef struct TwkTriangleAttributes
{
  float vertex[3];
  float tangent[3];
  float normal[3];
  float texcoord[3];
} TwkTriangleAttributes;

/* ≙ DeviceState, reference inc/Device.h:277-290 */
typedef struct TwkDeviceState
{
  int   resolution[2];
  int   tileSize[2];     /* power of two */
  int   pathLengths[2];  /* .x = min length before Russian roulette, .y = max length */
  int   distribution;    /* 1: checkerboard tile distribution over deviceCount devices */
  int   samplesSqrt;
  int   lensShader;
  float epsilonFactor;   /* sceneEpsilon = epsilonFactor * 1e-7 (config.h:42) */
  float envRotation;
  float clockFactor;     /* accepted, unused (USE_TIME_VIEW is 0 in the reference build) */
} TwkDeviceState;

/* Flattening (build option of twk_build, ≙ the accelBuildOptions of Device.cpp:1383-1389): an instance is FLATTENED
 * when its geometry has at most `maxTriangles` triangles (walls, light quads) or is referenced by at most
 * `maxReferences` instances (instancing saves no memory worth a per-ray instance entry). Flattened instances are
 * intersected in WORLD space: their vertices are transformed once at twk_build (row-major 3x4 object-to-world,
 * m0*x + m1*y + m2*z + m3 in fp32, as transformPoint closesthit.cu:88-98 evaluates it) and tested against the
 * untransformed ray, all in one world-space BVH; every other instance is entered through the top level with the ray
 * taken through the inverse transform (≙ IAS→GAS descent, Device.cpp:1427-1445). t, beta, gamma name the same
 * quantities either way; which one applies is part of the traversal contract the CPU oracle restates
 * (oracle/orc_trace.h), so both sides take the same policy. (0, 0) = pure two-level. */
#define TWK_FLATTEN_TRIANGLES  4
#define TWK_FLATTEN_REFERENCES 2

/* Texture slots ≙ the three hard-wired textures of Device::initTextures (Device.cpp:911-942). */
enum { TWK_TEXTURE_ALBEDO = 0, TWK_TEXTURE_CUTOUT = 1, TWK_TEXTURE_ENVIRONMENT = 2 };

/* Per-launch work counters (device side, exact integers). */
typedef struct TwkLaunchStats
{
  uint64_t radianceRays;    /* closest-hit rays traced */
  uint64_t shadowRays;      /* any-hit rays traced */
  uint64_t nodesVisited;    /* 4-ary wide nodes visited (64 B quantised records), both ray kinds */
  uint64_t trianglesTested; /* triangle records fetched (48 B each) */
  uint64_t instancesEntered;
  uint64_t shadedHits;
  uint64_t missed;
  uint64_t maxNodesPerRay;  /* longest single traversal (inner-node visits) seen by the wavefront trace kernel */
  uint64_t tailRays;        /* reserved (0): the persistent tail kernel of rounds 1-4 is an experiment patch now (tools/experiments/) */
  uint64_t tailNodesVisited;
  uint64_t tailTrianglesTested;
  uint64_t tailInstancesEntered;
  uint64_t overflowRays;    /* rays whose LDS traversal stack overflowed and were re-traced with the HBM-backed stack */
  uint64_t nodeWaveSteps;     /* wave-level iterations of the node step: lane occupancy there = nodesVisited / (64 * nodeWaveSteps) */
  uint64_t triangleWaveSteps; /* wave-level iterations of the triangle test */
  uint64_t leafWaveSteps;     /* wave-level executions of the leaf / instance entry / instance exit step */
  uint64_t cachedNodesVisited; /* of nodesVisited: wide nodes served from the LDS top-of-tree cache, not from memory */
  uint64_t droppedStackPushes; /* single-ray fallback traversal: pushes beyond its LDS + HBM stack (a truncated traversal); 0 on every scene tried */
  /* Where the waves of the persistent traversal kernel spend their time: shader-clock cycles (s_memtime, waits included)
   * summed over all waves, per phase of the kernel's outer loop — [0] refill (ray fetch), [1] node loop, [2] leaf /
   * instance step, [3] triangle loop, [4] pop + result write, [5] whole kernel. */
  uint64_t waveCycles[6];
  /* ABI 9. Where the waves of the shade kernel spend their instructions and their time, per phase of the shading of a path segment
   * (TWK_SHADE_PHASE_*): how often a wave ran the phase, with how many of its 64 lanes (lane occupancy of the phase = lanes /
   * (64 x wave steps)), and for how many shader-clock cycles (waits included). */
  uint64_t shadePhaseWaveSteps[24];
  uint64_t shadePhaseLanes[24];
  uint64_t shadePhaseCycles[24];
} TwkLaunchStats;
#define TWK_SHADE_PHASE_COUNT 24
/* index into TwkLaunchStats::shadePhase*: */
enum
{
  TWK_SHADE_PHASE_PATH = 0,          /* the whole shading of a segment */
  TWK_SHADE_PHASE_VOLUME_FETCH = 1,  /* volume stack top of a path inside a medium */
  TWK_SHADE_PHASE_MISS = 2,          /* miss programs (miss.cu) */
  TWK_SHADE_PHASE_HIT_RECORD = 3,    /* instance, shading record, material; normals; front face (closesthit.cu:126-186) */
  TWK_SHADE_PHASE_TANGENT = 4,       /* GGX materials: tangent */
  TWK_SHADE_PHASE_TEXCOORD = 5,      /* textured materials */
  TWK_SHADE_PHASE_LIGHT_HIT = 6,     /* implicit light hit (closesthit.cu:192-222) */
  TWK_SHADE_PHASE_BSDF_DIFFUSE = 7, TWK_SHADE_PHASE_BSDF_MIRROR = 8, TWK_SHADE_PHASE_BSDF_GLASS = 9,
  TWK_SHADE_PHASE_BSDF_GGX = 10, TWK_SHADE_PHASE_BSDF_GGX_GLASS = 11, /* the five sample callables */
  TWK_SHADE_PHASE_NEE_SAMPLE = 12,   /* draws + light sampler (closesthit.cu:252-264) */
  TWK_SHADE_PHASE_NEE_EVAL = 13,     /* BSDF eval + contribution (closesthit.cu:266-299) */
  TWK_SHADE_PHASE_RADIANCE = 14,     /* read-modify-write of the path's radiance */
  TWK_SHADE_PHASE_TAIL = 15,         /* integrator loop tail (raygeneration.cu:91-146) */
  TWK_SHADE_PHASE_VOLUME_PUSH = 16,  /* glass transmission: volume stack push / pop */
  TWK_SHADE_PHASE_AOV = 17,          /* denoiser AOV writes */
  TWK_SHADE_PHASE_KERNEL_LOAD = 18,  /* wait for the queue slot's streams */
  TWK_SHADE_PHASE_KERNEL_APPEND = 19,/* queue appends: ballots, barriers, the block's atomic, the stores (lanes = appending lanes) */
  TWK_SHADE_PHASE_KERNEL_ITERATION = 20, /* one block iteration of the kernel, per wave (lanes = lanes with a queue slot) */
  TWK_SHADE_PHASE_APPEND_BARRIER1 = 21,  /* of the append: from its start to behind the first barrier = the wait for the block's slowest wave */
  TWK_SHADE_PHASE_APPEND_ATOMIC = 22,    /* the round trip of the block's returning atomic, per issuing lane */
  TWK_SHADE_PHASE_APPEND_BARRIER2 = 23   /* from the first barrier to behind the second: stream requests, the atomic, the wait for it */
};

/* Accumulated device time per kernel class since twk_profile_reset (profiling mode only). */
enum
{
  TWK_KERNEL_GENERATE = 0,
  TWK_KERNEL_TRACE    = 1,
  TWK_KERNEL_SHADE    = 2,
  TWK_KERNEL_ACCUM    = 3,
  TWK_KERNEL_TAIL     = 4,  /* reserved: never launched by this build */
  TWK_KERNEL_COUNT    = 5
};

typedef struct TwkDevice_t* TwkDevice;

/* ---- seam 1/2: the per-GPU renderer ------------------------------------------------------- */

const char* twk_last_error(void);
int twk_abi_version(void);
int twk_device_count(int* count);

/* ≙ Device::Device(strategy, ordinal, index, count, miss, ...) — Device.cpp:222-317.
 * ordinal: HIP device ordinal. index/count: position in the set of rendering devices
 * (tile distribution). miss: 0 = black, 1 = constant white env, 2 = spherical HDR env
 * (selects the miss program like Device.cpp:660-672). */
int twk_device_create(TwkDevice* out, int ordinal, int index, int count, int miss);
int twk_device_destroy(TwkDevice dev); /* ≙ Device::~Device, Device.cpp:320-358 */

/* ≙ Device::setState, Device.cpp:1192-1256. May be called again on a live handle (a resized window, a re-tiling):
 *  - A state whose resolution, tileSize or distribution differs from the current one, or that gives another launchWidth, changes
 *    which pixel a launch index is and DISCARDS the handle's accumulations: its internal output, both AOVs, the luminance moments, the
 *    cascade's layers, the geometry AOV, the sample counts and the active and plan lists. They come back zeroed, at the new size, with
 *    the next call that needs them, as on a fresh handle; the picture restarts at iteration 0. The temporal history is dropped when
 *    the resolution changes. Path streams and scratch keep their capacity. A state that differs in nothing of these (path lengths,
 *    lens shader, epsilon, ...) allocates and clears nothing.
 *  - Device pointers obtained from twk_get_*_device_pointer must be fetched again after such a change; otherwise they are stable.
 *  - The padding of a packed tile buffer (distribution 1, several devices: launch indices whose column lies outside the picture)
 *    reads as zeros at all times, in every buffer of the handle: twk_estimate_noise counts it as empty and no list names it.
 *  - An external output buffer or shared frame (twk_set_output_device_pointer / twk_set_shared_frame) is the caller's: it is never
 *    cleared here, its stale words beyond the new picture included. One that is too small for the new state is let go: the handle
 *    accumulates into its internal buffer again, the caller's allocation is not written any more, and twk_get_output_device_pointer
 *    names the internal buffer; hand a large enough one in again after the call. */
int twk_set_state(TwkDevice dev, const TwkDeviceState* state);
int twk_init_cameras(TwkDevice dev, const TwkCameraDefinition* c, int count);   /* ≙ Device::initCameras   Device.cpp:944-968 */
int twk_init_lights(TwkDevice dev, const TwkLightDefinition* l, int count);     /* ≙ Device::initLights    Device.cpp:970-1000 */
int twk_init_materials(TwkDevice dev, const TwkMaterialGUI* m, int count);      /* ≙ Device::initMaterials Device.cpp:1002-1056 */
int twk_update_camera(TwkDevice dev, int idCamera, const TwkCameraDefinition* c);   /* ≙ Device::updateCamera   Device.cpp:1083-1096 */
int twk_update_light(TwkDevice dev, int idLight, const TwkLightDefinition* l);      /* ≙ Device::updateLight    Device.cpp:1098-1110 */
int twk_update_material(TwkDevice dev, int idMaterial, const TwkMaterialGUI* m);    /* ≙ Device::updateMaterial Device.cpp:1112-1168 */

/* ≙ Device::initTextures (Device.cpp:911-942). Texels are RGBA32F, row 0 = v 0 (origin lower left),
 * bilinear, normalized coordinates; wrap in u and v except the environment which clamps v
 * (Texture.cpp:668-693,1353). For TWK_TEXTURE_ENVIRONMENT the spherical CDFs and the integral
 * are computed like Texture::calculateSphericalCDF (Texture.cpp:1500-1645). */
int twk_init_texture(TwkDevice dev, int slot, const float* rgba, int width, int height);

/* Scene ≙ Device::initScene → traverseNode (Device.cpp:1058-1080,1283-1331), flattened by the caller. */
int twk_add_geometry(TwkDevice dev, const TwkTriangleAttributes* attributes, size_t numAttributes,
                     const unsigned int* indices, size_t numIndices, int* idGeometry); /* ≙ createGeometry (GAS) Device.cpp:1333-1425 */
int twk_add_instance(TwkDevice dev, int idGeometry, const float transform[12],
                     int idMaterial, int idLight, int* idInstance);                    /* ≙ createInstance Device.cpp:1427-1445 + hit record :1492-1532 */
int twk_build(TwkDevice dev);                                                          /* ≙ createTLAS + createHitGroupRecords Device.cpp:1448-1532 */
int twk_clear_scene(TwkDevice dev);
/* Acceleration-structure quality of the next twk_build (≙ the buildFlags of accelBuildOptions, Device.cpp:1383-1389):
 * TWK_BUILD_LBVH — Morton codes + radix tree, the fastest build; TWK_BUILD_SAH (default) — binned surface-area-heuristic
 * top-down splits, fewer node visits per ray. Hit records do not depend on it (closest hit is order independent). */
enum { TWK_BUILD_LBVH = 0, TWK_BUILD_SAH = 1 };
int twk_set_build_quality(TwkDevice dev, int quality);

/* What the last twk_build produced. SAH cost terms: over every bottom-level / flattened-instance tree, the sum of
 * half-area(node) / half-area(root of its tree) over the inner nodes that survive the leaf collapse (sahInnerCost)
 * and of half-area(leaf) / half-area(root) x triangles over its leaves (sahLeafCost): expected binary-node visits and
 * triangle tests of a random ray that hits the root box, summed over `trees` trees. */
typedef struct TwkBuildInfo
{
  int      quality;
  int      trees;
  double   sahInnerCost;
  double   sahLeafCost;
  double   buildMilliseconds; /* host wall time of twk_build, uploads included */
  uint64_t triangleSlots, nodes, instances, flattenedInstances;
  uint64_t maxTraversalDepth; /* ABI 4: binary-tree levels of the deepest root-to-leaf path (top level + the deepest tree below it); twk_build refuses a scene deeper than the traversal stacks */
  uint64_t directLeafInstances; /* ABI 5: flattened instances of at most a leaf's triangles that ARE leaves of the top level (no tree of their own is visited) */
  uint64_t traceBlocksPerCU;    /* ABI 5: resident blocks per CU of the persistent traversal kernel for this scene with the materials as they are now: 7 (every instance flattened, at most 1 M nodes — with or without cutout opacity), 5 (two-level with cutout opacity), else 6 */
  uint64_t wide8Nodes;          /* ABI 8: reserved, 0 — the compressed 8-ary nodes of round 4 lost on every scene and are an experiment patch now (tools/experiments/r04_wide8_nodes.patch) */
  uint64_t wide8Levels;         /* ABI 8: reserved, 0 */
  uint64_t pairLeaves;          /* leaves that hold a pair: triangles 2k, 2k + 1 of a geometry with the index triples (a, b, c), (c, d, a), built as one primitive (over every tree of the scene; 0 under TWK_TRIANGLE_PAIRS=0) */
  uint64_t pairTriangles;       /* triangle slots in those leaves: two each */
} TwkBuildInfo;
int twk_get_build_info(TwkDevice dev, TwkBuildInfo* info);

/* Layout of the path streams a wavefront pass over the built scene uses, with the materials as they are now. SLIM: every
 * instance is flattened and no material has cutout opacity — the instance of a hit rides in the hit record's slot word and
 * the launch index of a shadow ray in its pending record, 8 bytes less per path and bounce. FULL: every other scene, and
 * every scene under TWK_SLIM_STREAMS=0. The images are the same bit for bit. */
enum { TWK_STREAMS_FULL = 0, TWK_STREAMS_SLIM = 1 };
int twk_get_stream_layout(TwkDevice dev, int* layout);

/* Flattening policy of the next twk_build (defaults TWK_FLATTEN_TRIANGLES, TWK_FLATTEN_REFERENCES; see there). */
int twk_set_flatten_policy(TwkDevice dev, int maxTriangles, int maxReferences);

/* ≙ Device*::render(iterationIndex, buffer) → optixLaunch(pipeline, stream, d_sys, 192, &sbt, W, H, 1)
 * (DeviceSingleGPU.cpp:104-182; multi-GPU: DeviceMultiGPULocalCopy.cpp:104-190).
 * Asynchronous on the handle's stream. One call = one sample per pixel of this device's share:
 * the full W×H frame (distribution 0) or the launchWidth×H checkerboard tile set (distribution 1,
 * raygeneration.cu:152-164,259-344). The accumulation buffer holds the running mean
 * (raygeneration.cu:246-253), RGBA32F, alpha 1. After an adaptive pass (twk_launch_adaptive, below) an index other than 0 is
 * TWK_ERROR_INVALID_STATE, the pixels being at different iterations; index 0 restarts a uniform frame as always. */
int twk_launch(TwkDevice dev, unsigned int iterationIndex);
int twk_sync(TwkDevice dev);                                  /* ≙ Device::synchronizeStream */
/* twk_launch is asynchronous and deferred: consecutive iteration indices are rendered together, up to `iterations`
 * samples per pixel per wavefront pass (1..64, default 64; 280 bytes of path streams per sample and pixel), as soon
 * as the batch is full or any other call observes the device. The image is bit-identical to one pass per iteration; 1 restores strict one-launch-per-call behaviour. */
int twk_set_launch_batch(TwkDevice dev, int iterations);
/* The path streams of a pass are allocated on demand and grow with the largest pass seen; this allocates them up
 * front for passes of `iterations` samples per pixel, so that no allocation falls into a timed or interactive loop. */
int twk_reserve_launch_batch(TwkDevice dev, int iterations);

/* The two apps the hot path serves differ in ONE rule of __closesthit__radiance: rtigo3 ends a path on a light only
 * when its lit side is hit and lets a back-face hit fall through to the light's BSDF (apps/rtigo3/shaders/closesthit.cu:192-222);
 * Optix7Gui (intro_07's app) ends the path on either side, black on the back face (apps/Optix7Gui/shaders/closesthit.cu:189-226). */
enum { TWK_SHADERS_RTIGO3 = 0, TWK_SHADERS_OPTIX7GUI = 1 };
int twk_set_shader_variant(TwkDevice dev, int variant);

/* Denoiser AOVs of Optix7Gui's integrator (apps/Optix7Gui/shaders/raygeneration.cu:125-164,239-262), the input the
 * OptiX AI denoiser is fed with (the denoiser itself is closed third-party code and not part of this library):
 * TWK_AOV_ALBEDO: throughput-attenuated albedo of the first diffuse or light event, clamped to [0, 1], alpha 1;
 * TWK_AOV_NORMAL: shading normal of the primary hit in right-handed camera space, renormalised running mean, w 0.
 * Both accumulate like the radiance (running mean, skipped with it when a sample is NaN). Layout as twk_read_output. */
enum { TWK_AOV_ALBEDO = 0, TWK_AOV_NORMAL = 1 };
int twk_enable_aov(TwkDevice dev, int enable);
int twk_read_aov(TwkDevice dev, int which, float* rgbaHost, size_t numFloats);

/* Luminance moments of the integrator's samples, an AOV for the denoiser (twk_denoise_variance_sampled) — new calls, ABI stays 9.
 * While enabled, the kernel that folds a pass's samples into the running mean folds, in the same read, Welford's recurrence over
 * the luminance l = 0.2126 r + 0.7152 g + 0.0722 b of every sample it keeps (the ones the running mean keeps: NaN samples are
 * dropped, or replaced by their false colour under twk_set_debug_exceptions) — per sample, in iteration order, n = n + 1;
 * d = l - mean; mean = mean + d / n; M2 = M2 + d (l - mean) — into one float4 (mean, M2, n, 0) per launch index, laid out
 * like the AOVs (launchWidth x height, also under twk_set_shared_frame) and ALWAYS f32, in TWK_OUTPUT_HALF4 mode too (the square
 * of a half-range luminance does not fit a half). A kept sample of iteration 0 starts the triple afresh. M2 / (n - 1) is the
 * sample variance of the luminance, M2 / ((n - 1) n) the variance of the pixel's mean. A sample that is not finite makes the
 * triple not finite. The result does not depend on twk_set_launch_batch or on how a pass is cut into lanes. The operations and
 * their order: csrc/shade_device.h foldSamples. twk_enable_moments(1) allocates the buffer, zeroed (with twk_set_state, whichever
 * comes later); (0) frees it. With moments off nothing changes: the builds of the kernels without them run. */
int twk_enable_moments(TwkDevice dev, int enable);
int twk_read_moments(TwkDevice dev, float* host, size_t numFloats); /* launchWidth*height*4 floats; synchronises */
int twk_get_moments_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);

/* ABI 6. Time view, ≙ the reference's compile-time USE_TIME_VIEW (apps/rtigo3/shaders/config.h:60, raygeneration.cu:169-171,
 * 231-244, Device.h:350): while enabled the ALPHA of the accumulation buffer is not 1 but the running mean of
 * (shader-clock cycles the sample's lanes spent in traversal and shading) x TwkDeviceState::clockFactor x 1e-9 — what
 * rtigo3's rasteriser maps through its colour ramp. RGB is unchanged, bit for bit. The reference counts one thread's
 * clock() from ray generation to the write; a wavefront path has no single thread, so the cycles of its lanes in every
 * traversal and shade launch are summed (lanes of a wave wait for each other in both designs). Measurement builds of the
 * kernels run while it is on (as with twk_stats_enable): it is a diagnostic view, not a fast path. */
int twk_set_time_view(TwkDevice dev, int enable);

/* ABI 9. ≙ the reference's compile-time lighting switch USE_NEXT_EVENT_ESTIMATION (shaders/config.h:50-52), a run-time switch
 * here: 1 (default) = next-event estimation per path vertex with power-heuristic MIS; 0 = brute-force path tracing — no light
 * sample, no shadow ray (closesthit.cu:250-304), implicit light and environment hits unweighted (closesthit.cu:202-214,
 * miss.cu:62-68,92-106). Both estimate the same image; the reference keeps the switch "to compare lighting results". */
int twk_set_next_event_estimation(TwkDevice dev, int enable);
/* ABI 9. ≙ USE_DEBUG_EXCEPTIONS of the ray generation program (config.h:54-56, raygeneration.cu:205-218): 1 = a sample that is
 * NaN / infinite / negative is accumulated as super red / green / blue (1e6) instead of NaN samples being dropped; 0 (default). */
int twk_set_debug_exceptions(TwkDevice dev, int enable);

/* Output format of the accumulation and AOV buffers, ≙ Optix7Gui's compile-time USE_FP32_OUTPUT (apps/Optix7Gui/shaders/
 * app_config.h:57-59): TWK_OUTPUT_FLOAT4 (default) = RGBA32F, 16 B per pixel; TWK_OUTPUT_HALF4 = RGBA16F (Half4, 8 B per
 * pixel), the format of a GL_RGBA16F display texture and of OPTIX_PIXEL_FORMAT_HALF4 denoiser input. In half mode every
 * sample is folded as in float mode from the widened half (f32 arithmetic), then rounded to nearest even
 * (raygeneration.cu:267-317, half_common.h:36-80): what exceeds 65504 becomes +-inf. Switching synchronises the stream and
 * reallocates the internal output and AOV buffers, zeroed; setting the current format is a no-op; an external buffer
 * (twk_set_output_device_pointer / twk_set_shared_frame) too small for the new format is refused (TWK_ERROR_INVALID_STATE).
 * twk_read_output / twk_read_aov keep returning RGBA32F, widened exactly; twk_read_output_raw / twk_read_aov_raw return
 * the buffer's bytes in its format (bytes must be the pixel count times 16 or 8). */
enum { TWK_OUTPUT_FLOAT4 = 0, TWK_OUTPUT_HALF4 = 1 };
int twk_set_output_format(TwkDevice dev, int format);
int twk_get_output_format(TwkDevice dev, int* format);
int twk_read_output_raw(TwkDevice dev, void* host, size_t bytes);
int twk_read_aov_raw(TwkDevice dev, int which, void* host, size_t bytes);

/* Output. With distribution 0 the buffer is W×H (≙ outputBuffer); with distribution 1 it is the
 * packed launchWidth×H local tile buffer (≙ texelBuffer, DeviceMultiGPULocalCopy.cpp:109-172). */
int twk_get_launch_width(TwkDevice dev, int* launchWidth);    /* ≙ m_launchWidth, DeviceMultiGPULocalCopy.cpp:84-97 */
int twk_read_output(TwkDevice dev, float* rgbaHost, size_t numFloats); /* ≙ getOutputBufferHost, sync D2H */
int twk_get_output_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);
/* Let the caller own the accumulation buffer (device memory of ≥ launchWidth*H*16 B, 8 B per pixel in
 * TWK_OUTPUT_HALF4 mode, e.g. a torch tensor used as RCCL send buffer). Pass NULL to return to the internal buffer.
 * twk_get_output_device_pointer reports launchWidth*H times the pixel size of the output format. */
int twk_set_output_device_pointer(TwkDevice dev, void* dptr, size_t bytes);

/* The reference's two other multi-GPU buffer strategies (≙ DeviceMultiGPUZeroCopy.cpp:106-118: one pinned host buffer
 * mapped into every device; DeviceMultiGPUPeerAccess.cpp:110-158: one buffer on the first device, written by its peers):
 * every device accumulates straight into ONE shared W x H RGBA32F frame at the pixel its launch index maps to
 * (raygeneration.cu:175-183,229), no packed tile buffers, no compositor. `frame` must be addressable from this device
 * (hipHostMalloc(..., hipHostMallocPortable | hipHostMallocMapped), or device memory with peer access enabled);
 * devices write disjoint pixels. NULL returns to the internal packed buffer. twk_read_output then returns the frame. */
int twk_set_shared_frame(TwkDevice dev, void* frame, size_t bytes);

/* ≙ DeviceMultiGPULocalCopy::compositor + compositor.cu:38-64, for all source devices in one kernel:
 * `tiles` is the gathered [deviceCount][H][launchWidth] RGBA32F block (device memory, rank order),
 * `output` the full W×H RGBA32F image (device memory). Runs on this handle's stream. */
int twk_compositor(TwkDevice dev, const void* tiles, void* output);
/* The same for RGBA16F tiles into an RGBA16F W×H frame (TWK_OUTPUT_HALF4): a plain 8-byte copy per pixel. */
int twk_compositor_half(TwkDevice dev, const void* tiles, void* output);

/* ≙ TonemapperGUI (inc/TonemapperGUI.h:34-43), same field order. Neutral defaults: gamma 1, whitePoint 1,
 * colorBalance 1 1 1, burnHighlights 1, crushBlacks 0, saturation 1, brightness 1 (Application.cpp:111-120). */
typedef struct TwkTonemapper
{
  float gamma;
  float whitePoint;
  float colorBalance[3];
  float burnHighlights;
  float crushBlacks;
  float saturation;
  float brightness;
} TwkTonemapper;

/* ≙ the tonemapper loop of Application::screenshot (Application.cpp:2259-2297), as the device kernel its authors
 * ask for there: RGBA32F → RGB8, pixel i at rgb8Host[3*i..3*i+2], same row order as the input.
 * rgbaDevice NULL: the handle's own accumulation buffer (numPixels must be launchWidth*height); otherwise any
 * device buffer of numPixels float4 (e.g. the composited multi-GPU image). Synchronises the handle's stream. */
int twk_tonemap(TwkDevice dev, const TwkTonemapper* tm, const void* rgbaDevice, size_t numPixels, unsigned char* rgb8Host);
/* The handle's own buffer is tonemapped in whatever format it holds. twk_tonemap_half: an explicit device buffer of numPixels
 * RGBA16F pixels (e.g. a frame of twk_compositor_half), widened, then the same operator. */
int twk_tonemap_half(TwkDevice dev, const TwkTonemapper* tm, const void* rgbaHalfDevice, size_t numPixels, unsigned char* rgb8Host);

/* ---- denoiser ------------------------------------------------------------------------------ */
/* Stands at the seam of Optix7Gui's optixDenoiserInvoke (apps/Optix7Gui/src/Application.cpp:942-1001): beauty + albedo +
 * normal in, denoised picture out, then the tonemapper. The OptiX AI denoiser is a closed network; this is a CLASSICAL filter,
 * the edge-avoiding a-trous wavelet of Dammertz et al. 2010, guided by the same two AOVs and defined exactly (the float
 * operations and their order: csrc/denoise_device.h). Per level i = 0 .. iterations-1, step s = 1 << i, 5x5 B3-spline stencil
 * h = (1/16, 1/4, 3/8, 1/4, 1/16), k = h[dy] h[dx], taps outside the picture skipped:
 *   w = k exp(-(|c_p-c_q|^2/sigmaColor^2 + |n_p-n_q|^2/sigmaNormal^2 + |a_p-a_q|^2/sigmaAlbedo^2)),  c_p' = sum w c_q / sum w,
 * terms of guides not in use omitted, sigmaColor the same on every level. A tap with a non-finite colour or guide has weight 0;
 * a centre with a non-finite colour or guide (or whose demodulated colour overflows) passes through unchanged, as the input's
 * bits; alpha is always the input's.
 * ≙ OptixDenoiserOptions::inputKind + OptixDenoiserParams (Optix7Gui Application.cpp:2451-2505) */
enum { TWK_DENOISER_RGB = 0, TWK_DENOISER_RGB_ALBEDO = 1, TWK_DENOISER_RGB_ALBEDO_NORMAL = 2 };
typedef struct TwkDenoiser
{
  int   inputKind;        /* which guides weigh the taps (≙ USE_DENOISER_ALBEDO / USE_DENOISER_NORMAL, app_config.h) */
  int   iterations;       /* a-trous levels, step 1 << level; 0..8 */
  float sigmaColor, sigmaNormal, sigmaAlbedo;
  int   demodulateAlbedo; /* filter rgb / max(albedo, 0.01), multiply back afterwards; needs an albedo guide */
  float blendFactor;      /* ≙ OptixDenoiserParams::blendFactor: 0 = denoised only, 1 = input */
} TwkDenoiser;
/* RGB_ALBEDO_NORMAL, 3 iterations, sigmaColor 8, sigmaNormal 0.3, sigmaAlbedo 0.1, demodulateAlbedo 1, blendFactor 0 */
int twk_denoiser_defaults(TwkDenoiser* dn);
/* Asynchronous on the handle's stream; never writes its inputs. beauty NULL (then albedo and normal must be NULL too, and
 * width / height are ignored): the handle's own accumulation and AOV buffers, launchWidth x height, are filtered — guided
 * kinds need twk_enable_aov(1), and a packed tile buffer (distribution 1 with more than one device) is refused. Otherwise
 * beauty, and the guides the kind uses, are device buffers of width x height pixels in the handle's current output format
 * (e.g. a composited multi-GPU frame). denoised NULL: the result goes to an internal buffer in the output format (≙
 * m_d_denoisedBuffer; allocated on first use, again when the resolution or the format changes), which the three calls below
 * hand out; otherwise to the caller's buffer, which must not overlap an input. RGBA16F input is widened exactly, all
 * arithmetic and the buffers between levels are f32, the result is narrowed once, round to nearest even. iterations 0 or
 * blendFactor 1 copy the input's bits. */
int twk_denoise(TwkDevice dev, const TwkDenoiser* dn, const void* beauty, const void* albedo, const void* normal,
                int width, int height, void* denoised);
/* The variance-guided, firefly-clamping mode of the same filter: the spatial-variance path of Schied et al. 2017 (SVGF, sections
 * 4.2 and 4.4), which that paper uses where no temporal history exists. Between prepare and level 0 a moments pass estimates, per
 * pixel p, mean m1 and variance var of the luminance l = 0.2126 r + 0.7152 g + 0.0722 b over the 7x7 window around p, the centre
 * left out (a firefly must not vouch for itself), every tap weighted by the guide terms of the formula above alone. With
 * fireflyThreshold k > 0 a pixel whose luminance exceeds limit = m1 + k sqrt(var) > 0 has its rgb scaled by limit / l_p. In the
 * levels the colour term is replaced by |l_p - l_q| / (sigmaLuminance sqrt(v_p) + 1e-3), v_p the 3x3 binomial of the variance at
 * the level's step, and the variance is filtered along: var' = sum w^2 var_q / (sum w)^2. dn->sigmaColor is ignored. Everything
 * else — buffers, formats, pass-through, alpha, blendFactor, the copies at iterations 0 / blendFactor 1 — is twk_denoise's, and
 * the result goes to the same internal buffer. What it is: a spatial variance estimate from the picture itself, and a clamp that
 * biases bright isolated pixels downwards. What it is not: a learned filter, or one that knows the per-sample variance of the
 * integrator. The float operations and their order: csrc/denoise_device.h. */
typedef struct TwkDenoiserVariance
{
  float fireflyThreshold; /* k of the clamp, in standard deviations of the neighbourhood; 0 = no clamp; >= 0 and finite */
  float sigmaLuminance;   /* scale of the luminance edge-stop, in standard deviations; > 0 and finite */
} TwkDenoiserVariance;
/* fireflyThreshold 3, sigmaLuminance 4 */
int twk_denoiser_variance_defaults(TwkDenoiserVariance* dv);
int twk_denoise_variance(TwkDevice dev, const TwkDenoiser* dn, const TwkDenoiserVariance* dv, const void* beauty, const void* albedo,
                         const void* normal, int width, int height, void* denoised);
/* twk_denoise_variance with the MEASURED variance where the integrator has seen enough samples — SVGF's rule the other way
 * round: that paper falls back to the spatial estimate where it has no history, and a progressive renderer always has some.
 * `moments` holds width x height float4 (mean, M2, n, .) as twk_enable_moments accumulates them. In the moments pass, a pixel with
 * n >= minSamples, finite mean, M2 and n, and mean > 0 gets var = M2 / ((n - 1) n) x rho^2 x f^2 — the variance of the pixel's
 * mean, taken into the space the levels filter in: rho = l_p / mean with demodulateAlbedo (l_p the luminance of the demodulated
 * colour before the clamp), else 1; f the factor the firefly clamp scaled the pixel by, 1 without. Every other pixel keeps the
 * spatial estimate. The clamp itself stays spatial (a firefly must not vouch for itself). Everything else is
 * twk_denoise_variance's, bit for bit; with every pixel below minSamples the result is twk_denoise_variance's. beauty NULL (then
 * albedo, normal and moments must be NULL too): the handle's own buffers and its own moments — needs a render with
 * twk_enable_moments(1); a packed tile buffer is refused, and so is minSamples < 2. What it is not: a learned filter, a temporal
 * one (one frame's samples, no reprojection), or per-sample moments of the demodulated colour (rho rescales the moments of the
 * beauty's luminance). The float operations and their order: csrc/denoise_device.h. */
int twk_denoise_variance_sampled(TwkDevice dev, const TwkDenoiser* dn, const TwkDenoiserVariance* dv, int minSamples, const void* beauty,
                                 const void* albedo, const void* normal, const void* moments, int width, int height, void* denoised);
/* The geometry guide — new calls, ABI stays 9, TwkDenoiser stays 28 bytes, TwkDenoiserVariance does not grow. The geometric half of
 * SVGF's edge-stopping function (Schied et al. 2017, section 4.4) as a fourth guide of the three modes above: albedo and normal
 * cannot tell a white block from the white wall parallel to it; the world position of the first hit can. A tap is weighed by
 * exp(-(d / (sigmaPosition |gp - P|))^2), d its distance from the centre's tangent plane (the plane through the centre's world
 * position gp whose normal is the centre's normal guide taken back to world space), |gp - P| the centre's distance from the camera —
 * TwkTemporal::positionTolerance's convention. A hit and a miss never mix, and with instanceStop neither do two instances.
 * `geometry`: width x height float4, always f32, as twk_render_geometry writes them — (world position, bits of instance + 1), a miss
 * (0, 0, 0, bits 0); `camera`: the 12 floats P, U, V, W it was traced from (a TwkCameraDefinition's first 12), NULL: the handle's
 * camera 0. dv NULL: twk_denoise's mode; dv and minSamples 0: twk_denoise_variance's; dv and minSamples >= 2:
 * twk_denoise_variance_sampled's with `moments` (NULL otherwise). inputKind must be TWK_DENOISER_RGB_ALBEDO_NORMAL (else
 * TWK_ERROR_INVALID_VALUE), and 1 / sigmaPosition^2 a finite positive float; every other refusal is the mode's own.
 * beauty NULL (then every other input NULL): the handle's accumulation, AOVs, moments and geometry AOV — TWK_ERROR_INVALID_STATE
 * without twk_enable_geometry(1), with a geometry AOV older than the camera, the state or the scene (twk_render_geometry first), and
 * on a packed tile buffer. Explicit buffers: a NULL geometry, or one the denoised buffer overlaps, is TWK_ERROR_INVALID_VALUE. The
 * result goes where the three calls above put theirs. With a geometry of misses only the result is, bit for bit, that of the mode's
 * own call. What it is not: a depth-gradient stop, a guide for lenses other than the pinhole or for cutout scenes (the geometry AOV
 * refuses those), or a term of the firefly clamp's threshold. The float operations and their order: csrc/denoise_device.h. */
typedef struct TwkDenoiserGeometry
{
  float sigmaPosition; /* distance from the centre's tangent plane, relative to the centre's distance from the camera */
  int   instanceStop;  /* 1: a tap on another instance weighs 0 */
} TwkDenoiserGeometry;
#define TWK_DENOISER_SIGMA_POSITION 0.01f /* the pick of the sweep's rule: profiles/r20_denoise_geometry.md */
/* sigmaPosition TWK_DENOISER_SIGMA_POSITION, instanceStop 0 */
int twk_denoiser_geometry_defaults(TwkDenoiserGeometry* dg);
int twk_denoise_geometry(TwkDevice dev, const TwkDenoiser* dn, const TwkDenoiserGeometry* dg, const TwkDenoiserVariance* dv, int minSamples,
                         const void* beauty, const void* albedo, const void* normal, const void* moments, const void* geometry,
                         const float* camera, int width, int height, void* denoised);
/* twk_denoise_geometry on the host: no handle, RGBA32F host buffers, the same definition compiled for the host (all three modes;
 * camera must be given). How the definition is checked without a GPU. */
int twk_denoise_geometry_host(const TwkDenoiser* dn, const TwkDenoiserGeometry* dg, const TwkDenoiserVariance* dv, int minSamples,
                              const float* beauty, const float* albedo, const float* normal, const float* moments, const float* geometry,
                              const float* camera, int width, int height, float* denoised);
int twk_read_denoised(TwkDevice dev, float* rgbaHost, size_t numFloats);        /* RGBA32F, widened exactly, like twk_read_output */
int twk_read_denoised_raw(TwkDevice dev, void* host, size_t bytes);             /* in the output format */
int twk_get_denoised_device_pointer(TwkDevice dev, void** dptr, size_t* bytes); /* feeds twk_tonemap / twk_tonemap_half */

/* ---- The temporal seam — new calls, ABI stays 9, no existing struct changes -----------------------------------------------------
 * The temporal half of SVGF (Schied et al. 2017, section 4.1) in front of the filter above: after a camera move an interactive
 * viewer restarts at iteration 0 with a handful of samples; these calls reproject the last frame's colour and luminance moments
 * through the previous camera and merge them with the new frame's samples BY SAMPLE COUNT. The loop of a frame:
 *   twk_set_sample_offset(frames x spp); twk_launch 0 .. spp-1; twk_render_geometry; twk_temporal_accumulate;
 *   twk_denoise_variance_sampled on the merged colour and merged moments.
 * Everything is opt-in; with the switches at their defaults nothing changes. Definition: csrc/temporal_device.h. */

/* Default 0. While set, iteration i draws its random numbers as iteration i + offset does otherwise (the second argument of the
 * seed's tea<4>); everything that COUNTS samples is unchanged: the running mean's weight 1 / (i + 1), "iteration 0 starts
 * afresh", the moments' n. A frame restarted at iteration 0 after a camera move sets offset = frames x spp, so that its noise is
 * independent of the history it is merged with (without it, a pixel reprojected by less than a pixel meets its own random
 * sequence again). A run-time value of the launch parameters, not a kernel build. Recorded launches are rendered first. */
int twk_set_sample_offset(TwkDevice dev, unsigned int offset);

/* Geometry AOV: one float4 per launch index, laid out like the moments, always f32: (world position of the primary hit, bits of
 * (unsigned) instance + 1), or (0, 0, 0, bits 0) for a miss. twk_enable_geometry(1) allocates it, zeroed (with twk_set_state,
 * whichever comes later); (0) frees it. twk_render_geometry enqueues, on the handle's stream, ONE kernel that traces one
 * closest-hit ray through the CENTRE of every pixel (the pinhole lens shader with the jitter 0.5, the single-ray traversal of
 * twk_trace_rays, tmin = the scene epsilon) with the camera as it is now. TWK_ERROR_INVALID_STATE: before twk_build or
 * twk_set_state, with the geometry off, with a lens shader other than the pinhole (reprojection inverts the pinhole mapping
 * only), on a packed tile buffer (distribution 1, several devices), and on a scene with a cutout texture in use (the query is
 * geometric). */
int twk_enable_geometry(TwkDevice dev, int enable);
int twk_render_geometry(TwkDevice dev);
int twk_read_geometry(TwkDevice dev, float* host, size_t numFloats); /* launchWidth*height*4 floats (w: the bits of a uint); synchronises */
int twk_get_geometry_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);

/* maxHistory: the cap, in samples, on what the history weighs (>= 1): an old frame fades like an exponential average with
 * alpha = spp / (maxHistory + spp). positionTolerance: a history tap belongs to the surface point when their world positions
 * differ by at most positionTolerance x the point's distance to the previous camera (>= 0, finite). */
typedef struct TwkTemporal { int maxHistory; float positionTolerance; } TwkTemporal;
#define TWK_TEMPORAL_MAX_HISTORY 32
#define TWK_TEMPORAL_POSITION_TOLERANCE 0.01f
int twk_temporal_defaults(TwkTemporal* tp);
/* One frame's buffers, width x height elements each, device pointers: colour, luminance moments (mean, M2, n, .) as
 * twk_enable_moments accumulates them, geometry AOV, and the camera the frame was rendered from. */
typedef struct TwkTemporalFrame { const void* colour; const void* moments; const void* geometry; TwkCameraDefinition camera; } TwkTemporalFrame;
/* Asynchronous, one kernel on the handle's stream. Per pixel: the surface point of current->geometry is projected through
 * history->camera, the history's colour and moments are fetched bilinearly at the four pixels around it — those whose geometry
 * has the same instance word and lies within the tolerance, and whose values are finite with n >= 1 — the history's n is capped
 * at maxHistory (M2 scaled along), and the two sample sets are merged: colour by sample count, moments by Chan's pairwise form
 * of Welford. A pixel without history (a miss, a point behind or outside the previous view, no tap that belongs to it, values
 * that are not finite, n < 1) passes through with the input's bits. tp NULL: twk_temporal_defaults.
 * EXPLICIT form (current != NULL): current->colour is in the handle's output format (RGBA32F, or RGBA16F widened exactly),
 * everything else f32 float4; history->colour is a previous call's historyOut. history NULL: no history, every pixel passes
 * through. current->camera is not read (it is the next call's history->camera). colourOut: the merged colour in the output
 * format, narrowed once — what twk_denoise_variance_sampled is handed as beauty; historyOut: the same colour unrounded in f32;
 * momentsOut: the merged moments (mean, M2, n, 0). Any of the three may be NULL. TWK_ERROR_INVALID_VALUE: a NULL input, an output
 * that overlaps an input or another output (the kernel gathers history at other pixels), maxHistory < 1, a tolerance that is
 * negative or not finite, and a history camera whose U, V, W are linearly dependent or not finite.
 * OWN-BUFFER form (current and history NULL; width, height and the outputs must be 0 / NULL): current is the handle's
 * accumulation buffer, moments, geometry AOV and camera 0 — TWK_ERROR_INVALID_STATE unless twk_enable_moments,
 * twk_enable_geometry and a twk_render_geometry since the last camera, state or scene change, and on a packed tile buffer. The
 * history is what the previous call kept (f32 colour, moments, geometry, camera) in double-buffered streams of the handle,
 * allocated on first use and dropped by twk_temporal_reset, a change of resolution, twk_clear_scene and twk_build. The first call
 * after that has no history: it copies the frame through and keeps it. The results go to internal buffers:
 * twk_get_temporal_device_pointers (colour in the output format, merged moments f32; either pair may be NULL), twk_read_temporal
 * (RGBA32F, widened exactly) and twk_read_temporal_moments. What it is not: see csrc/temporal_device.h — motion of one matrix per
 * instance only, after twk_update_instance_transform ("Moving an object" below), no environment reprojection (a miss never has history), pinhole only; a frame tiled over several
 * devices is merged by twk_temporal_accumulate_assembled ("The temporal seam on several devices" below). */
int twk_temporal_accumulate(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                            int width, int height, void* colourOut, void* historyOut, void* momentsOut);
int twk_temporal_reset(TwkDevice dev);
int twk_get_temporal_device_pointers(TwkDevice dev, void** colour, size_t* colourBytes, void** moments, size_t* momentsBytes);
int twk_read_temporal(TwkDevice dev, float* rgbaHost, size_t numFloats);         /* launchWidth*height*4 floats; synchronises */
int twk_read_temporal_moments(TwkDevice dev, float* host, size_t numFloats);

/* ---- The temporal seam on several devices — new calls, ABI stays 9, no existing struct, enum or constant changes; without them no
 * kernel's code and no byte of any buffer changes -------------------------------------------------------------------------------
 * A frame tiled over N handles (distribution 1) through the same loop: every handle traces the geometry of its own tile share
 * (twk_render_geometry_tile), ONE twk_assemble_devices_with_geometry moves the planes and the geometry to the primary handle, and
 * twk_temporal_accumulate_assembled merges the assembled frame there and keeps the history there. The loop of a frame:
 *   on every handle: twk_update_camera(0); twk_set_sample_offset(frames x spp); twk_launch 0 .. spp-1; twk_render_geometry_tile;
 *   on the primary: twk_assemble_devices_with_geometry(OUTPUT | MOMENTS [| CASCADE]); twk_temporal_accumulate_assembled;
 *   twk_denoise_variance_sampled / twk_cascade_resolve on the merged buffers, as on one device.
 * Everything a single handle gives for the same cameras, byte for byte (the renderer seeds by absolute pixel, the assembly moves
 * bytes, the merge kernels are the same). INTEGRATION.md "The temporal seam on several devices". */

/* twk_render_geometry for a handle whose buffers are packed tile buffers (distribution 1, several devices): ONE kernel, one element
 * per launch index i = ly * launchWidth + lx. Its pixel column is x = twk_tile_column(lx, ly, tileSize, count, index); x >= width is
 * padding and is written as a miss, (0, 0, 0, bits 0), without a ray; otherwise the ray through the centre of pixel (x, ly) is traced
 * exactly as twk_render_geometry traces it and the same value is written to element i (twk_read_geometry,
 * twk_get_geometry_device_pointer: launchWidth x height float4). On any other handle it IS twk_render_geometry. Refusals
 * (TWK_ERROR_INVALID_STATE): those of twk_render_geometry except the packed tile buffer — before twk_build or twk_set_state, the
 * geometry off, a lens shader other than the pinhole, a cutout texture in use. Definition: csrc/temporal_device.h. */
int twk_render_geometry_tile(TwkDevice dev);

/* twk_temporal_accumulate's own-buffer form on a tiled primary handle, with the planes it assembled as the current frame: colour =
 * the assembled TWK_PLANE_OUTPUT, moments = the assembled TWK_PLANE_MOMENTS, geometry = the assembled geometry AOV
 * (twk_assemble_with_geometry / twk_assemble_devices_with_geometry), camera = the primary's camera 0, width x height = the
 * picture's. The history is the handle's own temporal state, which a tiled handle does not use otherwise, so the result is handed
 * out by the existing calls, as width x height pixels: twk_get_temporal_device_pointers, twk_read_temporal,
 * twk_read_temporal_moments; twk_temporal_reset drops it, and the first call after a reset or a resize copies the frame through.
 * While twk_temporal_enable_cascade(1) is set on the primary it also merges the assembled TWK_PLANE_CASCADE layers
 * (twk_get_temporal_cascade_device_pointer, twk_read_temporal_cascade: [layers][height][width]). No kernel of its own: the merge
 * kernels run unchanged on W x H buffers. tp NULL: twk_temporal_defaults.
 * TWK_ERROR_INVALID_VALUE: a NULL handle (before any HIP call), maxHistory < 1, a tolerance that is negative or not finite.
 * TWK_ERROR_INVALID_STATE: before twk_set_state and twk_init_cameras; a handle that is not tiled (use twk_temporal_accumulate);
 * moments or geometry off; cascade merging on without twk_enable_cascade; TWK_PLANE_OUTPUT, TWK_PLANE_MOMENTS, (with cascade
 * merging) TWK_PLANE_CASCADE or the geometry not assembled, and an assembled geometry that is stale (the primary's camera, state
 * or scene changed since) — the text names which. */
int twk_temporal_accumulate_assembled(TwkDevice primary, const TwkTemporal* tp);

/* ---- The noise estimate and the stopping rule — new calls, ABI stays 9, no existing struct changes -----------------------------
 * How far a progressive picture is from done, from the integrator's own samples: per launch index the RELATIVE STANDARD ERROR of
 * the luminance mean, e = sqrt(M2 / ((n - 1) n)) / (mean + darkFloor), out of the luminance moments (mean, M2, n, .) that
 * twk_enable_moments accumulates, reduced on the device to a summary of integers. The complete definition, operation by
 * operation, is csrc/noise_device.h; tests/noise_restate.py restates it in numpy. An element is EMPTY (n == 0: the padding of a
 * packed tile buffer, a pixel whose samples were all dropped), UNKNOWN (a component that is not finite, n < minSamples, M2 < 0,
 * mean < 0, or an e that is not finite) or VALID. Valid elements are counted into histogram[256] by the exponent and the top three
 * mantissa bits of e (8 bins per octave from 2^-16 to 2^16, clamped), summed in units of 2^-20 (e capped at 65536) into sumFixed,
 * and the largest bits of e are kept: integers only, so the summary does not depend on the order of the reduction and equals its
 * restatement exactly. What it is NOT: an error against ground truth. It is blind to bias (the firefly clamp, clamped or cut
 * paths), it is not a measure of a denoised picture, and it sees luminance, not colour. */
typedef struct TwkNoise { int minSamples; float darkFloor; } TwkNoise;
#define TWK_NOISE_DARK_FLOOR 0.01f
int twk_noise_defaults(TwkNoise* np); /* minSamples TWK_DENOISER_MIN_SAMPLES, darkFloor TWK_NOISE_DARK_FLOOR */
typedef struct TwkNoiseSummary { uint64_t valid, unknown, empty, sumFixed; uint32_t maxErrorBits, reserved; uint32_t histogram[256]; } TwkNoiseSummary;
/* Estimates into the handle's summary buffer; asynchronous on the handle's stream (the summary is zeroed on that stream first), never
 * writes its input. np NULL: the defaults. moments NULL (numElements must be 0 then): the handle's own moments, launchWidth x height
 * elements — TWK_ERROR_INVALID_STATE without twk_enable_moments(1) and twk_set_state; ALLOWED on a packed tile buffer (distribution
 * 1, several devices), whose padding is EMPTY: each device reduces its own buffer and the host merges, no picture is assembled.
 * Recorded launches are rendered first. Otherwise moments is a device buffer of numElements float4. errorMap: NULL, or a device
 * buffer of numElements floats that does not overlap moments; it receives e for a VALID element, -1 for UNKNOWN, -2 for EMPTY.
 * TWK_ERROR_INVALID_VALUE: a NULL handle, minSamples < 2, a darkFloor that is not > 0 and finite, an overlap, numElements that is
 * not 0 without moments, or is 0 or above 2^31 with them. */
int twk_estimate_noise(TwkDevice dev, const TwkNoise* np, const void* moments, size_t numElements, void* errorMap);
int twk_read_noise(TwkDevice dev, TwkNoiseSummary* out); /* the last estimate's summary; synchronises. TWK_ERROR_INVALID_STATE before any estimate on this handle */
/* Host only, no handle. Merge: two summaries of disjoint element sets — counts, histogram and sumFixed add, maxErrorBits is the
 * larger. Mean: sumFixed / 2^20 / valid in double, narrowed once. Quantile, q in (0, 1]: the UPPER edge of the first bin at which
 * the cumulative count reaches ceil(q valid) (the ceiling in exact integer arithmetic), the float whose bits are
 * (bin + 1 + ((127 - 16) << 3)) << 20 — never below the true quantile and at most 9/8 of it inside the histogram's range. Mean and
 * quantile are TWK_ERROR_INVALID_STATE where valid == 0. */
int twk_noise_merge(TwkNoiseSummary* into, const TwkNoiseSummary* other);
int twk_noise_mean(const TwkNoiseSummary* s, float* mean);
int twk_noise_quantile(const TwkNoiseSummary* s, float q, float* error);

/* ---- Adaptive sampling — new calls, ABI stays 9, no existing struct changes; with the switch at its default no kernel and no bit
 * of any picture changes --------------------------------------------------------------------------------------------------------
 * Samples only the pixels the noise estimate says are unfinished. Paths of different pixels never interact, and the iteration index
 * enters a path in two places only: the seed of its random numbers and the fold into the running means (weight 1 / (iteration + 1),
 * "iteration 0 starts afresh", the moments). So every launch index i gets a word count[i], the iteration index its next sample uses,
 * and an adaptive sample of i uses count[i] wherever a uniform launch uses its iteration index. INVARIANT: after any mix of uniform
 * launches 0 .. K-1 and adaptive passes, a launch index whose count is c holds in colour, both AOVs and moments exactly the bits it
 * holds after twk_launch(0 .. c-1). What it is NOT: it does not predict how many samples a pixel still needs (every selected pixel
 * gets the same number per pass), it is driven by the luminance estimate above and so by neither colour, the denoised picture nor
 * bias, and an adaptive pass uses neither the fused primary builds nor several lanes. */
typedef struct TwkAdaptive { float targetNoise; int minSamples; float darkFloor; unsigned int maxSamples; } TwkAdaptive;
#define TWK_ADAPTIVE_TARGET_NOISE 0.05f
#define TWK_ADAPTIVE_MAX_SAMPLES 4096u
int twk_adaptive_defaults(TwkAdaptive* ap); /* targetNoise 0.05, minSamples TWK_DENOISER_MIN_SAMPLES, darkFloor TWK_NOISE_DARK_FLOOR, maxSamples 4096 */
/* (1) allocates count[], the active list and the select's scan scratch, launchWidth x height words each (with twk_set_state, whichever
 * comes later); (0) frees them and forgets the adaptive state. TWK_ERROR_INVALID_STATE: (1) without twk_enable_moments(1). The
 * handle remembers the index after the last iteration a uniform launch rendered; before count[] is first read it is filled with
 * that index. twk_set_state, twk_build, twk_clear_scene, a change of the output format or of the output buffer, twk_enable_moments
 * and twk_enable_adaptive(0) drop that memory and the active list. */
int twk_enable_adaptive(TwkDevice dev, int enable);
/* Selects, in ascending order, the elements an adaptive pass is to sample, and synchronises; *numActive receives their number.
 * Element i with (mean, M2, n, .) = moments[i] is classified as by twk_estimate_noise with minSamples and darkFloor; the tests are
 * applied in this order: EMPTY, not selected; counts[i] >= maxSamples, not selected; UNKNOWN, selected; VALID, selected exactly
 * when e > targetNoise. The complete definition is csrc/adaptive_device.h; tests/adaptive_restate.py restates it in numpy. Never
 * writes its inputs. ap NULL: the defaults. Own-buffer form (moments, counts, activeOut NULL, numElements 0): the handle's moments,
 * counts and list, the list twk_launch_adaptive renders; recorded launches are rendered first; ALLOWED on a packed tile buffer
 * (distribution 1, several devices), whose padding is EMPTY. Explicit form: device buffers of numElements float4, numElements words
 * and, for the list, numElements words that overlap neither. TWK_ERROR_INVALID_VALUE: a NULL handle or numActive (before any HIP
 * call), a targetNoise or darkFloor that is not > 0 and finite, minSamples < 2, maxSamples 0, an overlap, some but not all of the
 * three pointers, numElements that is not 0 without them, or is 0 or above 2^31 with them. TWK_ERROR_INVALID_STATE: the own-buffer
 * form without twk_enable_moments(1), twk_enable_adaptive(1) and twk_set_state. */
int twk_adaptive_select(TwkDevice dev, const TwkAdaptive* ap, const void* moments, const void* counts, size_t numElements,
                        void* activeOut, unsigned int* numActive);
/* Host only, no handle: the same definition over host arrays (numElements x 4 floats, numElements words; activeOut holds
 * numElements words). TWK_ERROR_INVALID_VALUE: a NULL array, the parameter refusals above, numElements above 2^31. */
int twk_adaptive_select_host(const TwkAdaptive* ap, const float* moments, const uint32_t* counts, size_t numElements,
                             uint32_t* activeOut, size_t* numActive);
/* Renders `samples` samples of every launch index of the handle's active list as one wavefront pass, asynchronously: sample s of
 * launch index i runs as iteration count[i] + s (seeded with twk_set_sample_offset's offset added, as a uniform launch is), is
 * folded by the uniform pass's own fold, and count[i] advances by `samples` (so a count may pass maxSamples by less than `samples`).
 * The list stays valid: the same list may be rendered again. A list of length 0 is a successful no-op. After the first adaptive pass
 * twk_launch with an index other than 0 is TWK_ERROR_INVALID_STATE; twk_launch with index 0 restarts a uniform frame. TWK_ERROR_INVALID_VALUE:
 * a NULL handle, samples outside 1..64. TWK_ERROR_INVALID_STATE: before an own-buffer twk_adaptive_select on this handle; after
 * anything that dropped the list (a twk_launch, twk_set_state, twk_build, twk_clear_scene, a change of format or output buffer);
 * with the time view, first-hit capture or statistics on; with twk_set_shared_frame in use. */
int twk_launch_adaptive(TwkDevice dev, int samples);
int twk_read_sample_counts(TwkDevice dev, uint32_t* host, size_t numElements); /* launchWidth*height words; synchronises. TWK_ERROR_INVALID_STATE without twk_enable_adaptive(1) and twk_set_state */
int twk_get_sample_counts_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);
/* The active list of the last own-buffer select: *numActive entries into host, which holds `capacity` words (host NULL and capacity
 * 0: the length alone); synchronises. TWK_ERROR_INVALID_VALUE: capacity below the length. TWK_ERROR_INVALID_STATE: no valid list. */
int twk_read_active(TwkDevice dev, uint32_t* host, size_t capacity, unsigned int* numActive);

/* ---- Planned adaptive pass — new calls, ABI stays 9, no existing struct changes; twk_adaptive_select, twk_launch_adaptive and their
 * kernels are what they were, and without these calls no bit of any picture changes -------------------------------------------------
 * Gives each unfinished launch index the samples its own noise estimate predicts. e is the standard error of a mean of n samples and
 * falls as 1 / sqrt(n), so an element at e reaches the target at about n (e / target)^2 samples: its budget for one pass is that
 * number less n, within [minBatch, maxBatch] and the room maxSamples leaves. One twk_adaptive_plan turns moments and counts into the
 * active list and, per entry, the offset of its first path; one twk_launch_adaptive_planned renders the sum of the budgets as ONE
 * wavefront pass. The INVARIANT above holds: a launch index whose count is c holds exactly the bits of twk_launch(0 .. c-1). What it
 * is NOT: a guarantee (the estimate is low where samples are few, so early plans under-allocate and the next plan corrects them), and
 * it is driven by the luminance estimate, so by neither colour, the denoised picture nor bias.
 * minBatch, maxBatch: 1 <= minBatch <= maxBatch <= 64 (twk_launch_adaptive's own limit). The defaults (TWK_DENOISER_MIN_SAMPLES: one
 * pass makes an element without an estimate classifiable; 64) are PROVISIONAL: chosen by reasoning, not yet by a measured sweep. */
typedef struct TwkAdaptivePlan { uint32_t minBatch; uint32_t maxBatch; } TwkAdaptivePlan;
int twk_adaptive_plan_defaults(TwkAdaptivePlan* plan); /* minBatch TWK_DENOISER_MIN_SAMPLES, maxBatch 64 (provisional) */
/* Plans, and synchronises once. Element i is in the plan exactly when twk_adaptive_select selects it for the same `ap`; its budget b:
 * UNKNOWN -> minBatch; VALID -> r = e / targetNoise, q = r r, need = n q, extra = need - n (float32, one rounding each),
 * b = !(extra < maxBatch) ? maxBatch : ceilf(extra), then max(b, minBatch); last b = min(b, maxSamples - counts[i]). The complete
 * definition is csrc/adaptive_plan_device.h; tests/adaptive_plan_restate.py restates it in numpy. activeOut receives the planned i in
 * ascending order (*numActive of them), pathOffsetOut the exclusive prefix sum of their budgets and, at [*numActive], *numPaths: entry k
 * owns paths pathOffsetOut[k] .. pathOffsetOut[k + 1] - 1. Never writes its inputs. ap, plan NULL: the defaults. Own-buffer form
 * (moments, counts, activeOut, pathOffsetOut NULL, numElements 0): the handle's moments and counts, and a list and offsets of the
 * plan's OWN (not twk_read_active's list: a plan leaves the last select's list valid), which twk_launch_adaptive_planned renders;
 * recorded launches are rendered first; allowed on a packed tile buffer, whose padding is EMPTY and gets budget 0. Explicit form:
 * device buffers of numElements float4, numElements words, and for the outputs numElements and numElements + 1 words.
 * TWK_ERROR_INVALID_VALUE: a NULL handle, numActive or numPaths (before any HIP call), the parameter refusals of twk_adaptive_select,
 * a plan outside 1 <= minBatch <= maxBatch <= 64, an output that overlaps an input or the other output, some but not all of the four
 * pointers, numElements that is not 0 without them, or is 0 or above 2^31 with them, and a plan of more than INT_MAX paths (the message
 * names both totals, which are still handed out; a wavefront pass counts its paths in an int). TWK_ERROR_INVALID_STATE: the own-buffer
 * form without twk_enable_moments(1), twk_enable_adaptive(1) and twk_set_state. */
int twk_adaptive_plan(TwkDevice dev, const TwkAdaptive* ap, const TwkAdaptivePlan* plan, const void* moments, const void* counts, size_t numElements,
                      void* activeOut, void* pathOffsetOut, unsigned int* numActive, unsigned long long* numPaths);
/* Host only, no handle: the same definition over host arrays (numElements x 4 floats, numElements words; activeOut holds numElements
 * words, pathOffsetOut numElements + 1). TWK_ERROR_INVALID_VALUE: a NULL array, the parameter and plan refusals above, numElements
 * above 2^31, more than INT_MAX paths. */
int twk_adaptive_plan_host(const TwkAdaptive* ap, const TwkAdaptivePlan* plan, const float* moments, const uint32_t* counts, size_t numElements,
                           uint32_t* activeOut, uint32_t* pathOffsetOut, size_t* numActive, unsigned long long* numPaths);
/* Renders the handle's plan as one wavefront pass of numPaths paths, asynchronously: sample s of entry k runs as iteration
 * count[active[k]] + s, is folded by the uniform pass's own fold in that order, and the count advances by the entry's budget. The
 * counts advance, so a plan is rendered ONCE: a second call without a new plan is TWK_ERROR_INVALID_STATE (an empty plan is a
 * successful no-op and stays). A twk_launch, an own-buffer twk_adaptive_select and everything that drops the active list drop the
 * plan. A twk_launch_adaptive does NOT: a plan rendered after it runs at the counts as they then are (the invariant holds), with the
 * budgets computed before it, so a count may pass maxSamples by that pass's samples. The other refusals are twk_launch_adaptive's. */
int twk_launch_adaptive_planned(TwkDevice dev);
/* The plan of the last own-buffer twk_adaptive_plan: *numActive entries into active (capacity words) and *numActive + 1 into pathOffset
 * (capacity + 1 words); both NULL and capacity 0: the two totals alone; synchronises. TWK_ERROR_INVALID_VALUE: capacity below the
 * length, one buffer without the other. TWK_ERROR_INVALID_STATE: no valid plan (none made, dropped, or already rendered). */
int twk_read_plan(TwkDevice dev, uint32_t* active, uint32_t* pathOffset, size_t capacity, unsigned int* numActive, unsigned long long* numPaths);

/* ---- The firefly cascade — new calls, ABI stays 9, no existing struct changes; with the switch at its default no kernel and no bit
 * of any picture, AOV, moments word or list changes ------------------------------------------------------------------------------
 * A firefly-robust estimate in front of the denoiser: the cascaded framebuffer of Zirr, Hanika and Dachsbacher, "Re-weighting
 * firefly samples for improved finite-sample Monte Carlo estimates" (CGF 2018). The accumulate kernels split every kept sample by
 * its luminance over `layers` brightness layers with thresholds start, start base, start base^2, ... (per-layer sums, K float4 per
 * launch index, layer-major [K][launchWidth x height], always f32; layer 0 .w = n, layer K-1 .w = samples rejected as not finite);
 * twk_cascade_resolve then counts a layer only as far as enough samples landed in it, in the pixel and its eight neighbours:
 * out = (layer 0 + sum_j w_j layer j) / n, w_j = min(1, c_j / kappa). With more samples every weight goes to 1 and the picture is
 * the plain mean. The complete definition is csrc/cascade_device.h; tests/cascade_restate.py restates it in numpy. What it is NOT:
 * learned, colour-aware (the reliability is of the luminance), temporal by itself (the layers are carried over a camera move by "The
 * cascade through the temporal merge" below, opt-in), or unbiased at finite n (the clamp above the top layer and every w_j < 1
 * remove energy); of the paper it leaves out the local/global mixing and the variance term. The running mean, the AOVs, the moments, the noise estimate and the adaptive passes do not see it. */
typedef struct TwkCascade { int layers; float start; float base; } TwkCascade;
typedef struct TwkCascadeResolve { float kappa; } TwkCascadeResolve;
#define TWK_CASCADE_LAYERS 6
#define TWK_CASCADE_START 1.0f
#define TWK_CASCADE_BASE 8.0f
#define TWK_CASCADE_KAPPA 32.0f /* PROVISIONAL: chosen by the sweep in profiles/r15_cascade.md, at the upper edge of its range */
int twk_cascade_defaults(TwkCascade* cp);                /* layers 6, start 1, base 8 */
int twk_cascade_resolve_defaults(TwkCascadeResolve* rp); /* kappa TWK_CASCADE_KAPPA (provisional) */
/* (1) turns the CASCADE builds of the accumulate kernels on and allocates the layers, zeroed (with twk_set_state, whichever comes
 * later); cp NULL: the defaults. (0) frees them (cp is ignored). The layers are zeroed wherever the moments are (a new allocation),
 * when the number of launch indices changes, and by a change of parameters while enabled; the same parameters again change nothing.
 * A kept sample of iteration 0 starts its launch index afresh. Needs neither the moments nor adaptive sampling; adaptive passes
 * fold into the layers like uniform ones. TWK_ERROR_INVALID_VALUE: a NULL handle, layers outside 2..8, a start that is not > 0 and
 * finite, a base that is not > 1 and finite, thresholds that reach inf. */
int twk_enable_cascade(TwkDevice dev, int enable, const TwkCascade* cp);
/* The layers, [layers][launchWidth*height] float4; recorded launches are rendered first; the read synchronises.
 * TWK_ERROR_INVALID_STATE without twk_enable_cascade(1) and twk_set_state. */
int twk_read_cascade(TwkDevice dev, float* host, size_t numFloats); /* numFloats = layers*launchWidth*height*4 */
int twk_get_cascade_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);
/* Resolves; asynchronous on the handle's stream, never writes its input. cp, rp NULL: the defaults. Own-buffer form (layers NULL,
 * width and height 0, resolved NULL): the handle's layers, which cp must describe (NULL: the parameters they were enabled with),
 * into the handle's internal resolved buffer in the output format (twk_get_resolved_device_pointer, twk_read_resolved); recorded
 * launches are rendered first. TWK_ERROR_INVALID_STATE without
 * twk_enable_cascade(1) and twk_set_state, and on a packed tile buffer (distribution 1 with several devices: the 3x3 window would
 * cross tile borders — assemble every layer with twk_compositor and use the explicit form). Explicit form: `layers` a device buffer
 * of [cp->layers][width*height] float4, `resolved` a device buffer of width*height pixels of the handle's output format that does
 * not overlap it. TWK_ERROR_INVALID_VALUE: a NULL handle (before any HIP call), the parameter refusals of twk_enable_cascade, a
 * kappa that is not > 0 and finite, an overlap, layers without a size or a resolved buffer, a size without layers, cp that
 * differs from the handle's own parameters in the own-buffer form, width*height above 2^28. */
int twk_cascade_resolve(TwkDevice dev, const TwkCascade* cp, const TwkCascadeResolve* rp, const void* layers, int width, int height, void* resolved);
/* The internal resolved picture of the last own-buffer twk_cascade_resolve: launchWidth*height pixels of the output format. The
 * pointer feeds twk_tonemap, twk_tonemap_half and the explicit `beauty` of the three twk_denoise* calls unchanged.
 * twk_read_resolved: RGBA32F, an RGBA16F picture widened exactly; synchronises. TWK_ERROR_INVALID_STATE before such a resolve. */
int twk_get_resolved_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);
int twk_read_resolved(TwkDevice dev, float* rgbaHost, size_t numFloats);
/* Host only, no handle: the same definition over host arrays. Fold: `samples` is [numSamples][numElements] x 4 floats (radiance rgb,
 * w == 0: the element has no sample there, as twk_debug_read_path_radiance gives them), sample s at iteration firstIteration + s;
 * a sample with a NaN component is dropped unless debugExceptions, which folds the false colours of twk_set_debug_exceptions; layers
 * is [cp->layers][numElements] x 4 floats, read and written. Resolve: layers as above with numElements = width*height; resolved
 * receives width*height x 4 floats, NOT narrowed. TWK_ERROR_INVALID_VALUE: a NULL array, the parameter refusals above. */
int twk_cascade_fold_host(const TwkCascade* cp, const float* samples, size_t numSamples, size_t numElements, unsigned int firstIteration,
                          int debugExceptions, float* layers);
int twk_cascade_resolve_host(const TwkCascade* cp, const TwkCascadeResolve* rp, const float* layers, int width, int height, float* resolved);

/* ---- The cascade through the temporal merge — new calls, ABI stays 9, no existing struct changes; with the switch at its default no
 * kernel and no bit of any output changes ---------------------------------------------------------------------------------------
 * twk_temporal_accumulate carries the plain mean over a camera move: a firefly that enters its history stays for up to maxHistory
 * samples, smeared along the reprojection path; and the cascade restarts at iteration 0, where a 3x3 window of a 1 - 4 spp frame
 * holds too few samples for any bright layer to be trusted. These calls reproject the cascade's per-layer SUMS the way the plain
 * mean is reprojected — the same projection, the same four taps, the same test of a tap's geometry, the same cap — and add them to
 * the frame's. Sums merge linearly: the result is again a cascade, luminance(layer j) / b[j] still counts samples, and
 * twk_cascade_resolve runs on it unchanged with the history's counts behind its weights. The loop of a frame:
 *   twk_set_sample_offset; twk_launch 0 .. spp-1; twk_render_geometry; twk_temporal_accumulate (with twk_temporal_enable_cascade(1));
 *   twk_cascade_resolve on the merged layers (explicit form); twk_denoise_variance_sampled with the resolved picture as beauty and
 *   the merged moments.
 * The complete definition is csrc/temporal_cascade_device.h; tests/temporal_cascade_restate.py restates it in numpy. What it is: a
 * linear, capped, bilinear carry-over of sums and counts. What it is NOT: exact counting — n (layer 0 .w) becomes a weighted, capped
 * count that is no integer, and the interpolation mixes the counts of neighbouring pixels; alpha and the luminance moments stay the
 * existing merge's business; motion of one matrix per instance only ("Moving an object" below), no environment reprojection (a miss never has history), pinhole only (tiles: the
 * assembled layers of a tiled frame go through twk_temporal_accumulate_assembled); the paper's variance term is not reprojected; the noise estimate and the adaptive passes do not see the merged layers. */

/* EXPLICIT form; asynchronous, one kernel on the handle's stream. currentLayers, historyLayers and layersOut are device buffers of
 * [cp->layers][width*height] float4 (the shape twk_get_cascade_device_pointer hands out and twk_cascade_resolve takes),
 * currentGeometry and historyGeometry width*height float4 geometry AOVs, historyCamera the camera the history was rendered from. A
 * pixel without history (a miss, a position that is not finite, a frame count layer 0 .w that is not finite or < 1, a point behind
 * or outside the previous view, no tap that belongs to it with a finite count >= 1 and a weight > 0) passes through with the input's
 * bits. historyLayers NULL (historyGeometry and historyCamera are then not read): every pixel passes through. layersOut is the next
 * call's historyLayers. tp, cp NULL: twk_temporal_defaults, twk_cascade_defaults. TWK_ERROR_INVALID_VALUE: a NULL handle (before any
 * HIP call), NULL current layers, current geometry or output, history layers without their geometry or camera, an output that overlaps
 * an input (the kernel gathers the history at other pixels), the parameter refusals of twk_enable_cascade, maxHistory < 1, a
 * tolerance that is negative or not finite, a history camera whose U, V, W are linearly dependent or not finite, width or height
 * < 1, width*height above 2^28. */
int twk_temporal_accumulate_cascade(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                    const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera,
                                    int width, int height, void* layersOut);
/* OWN-BUFFER form: a switch, default 0. While it is on, the own-buffer twk_temporal_accumulate ALSO merges the handle's cascade
 * layers, with its own tp, the previous geometry and camera it reprojects the plain mean with, before it swaps its history; its
 * colour and moments are byte for byte what they are with the switch off. The merged layers go to double-buffered layers of the
 * handle, allocated on first use; they are dropped by whatever drops the temporal history (twk_temporal_reset, a change of
 * resolution or output format, twk_clear_scene, twk_build), by twk_enable_cascade(0) or with new parameters, and by this switch going
 * off. The first call after a drop has no history of layers: it copies the frame's layers through and keeps them.
 * TWK_ERROR_INVALID_STATE: (1) without twk_enable_cascade(1); and the own-buffer twk_temporal_accumulate, beside its own refusals,
 * while the switch is on and the cascade is off. */
int twk_temporal_enable_cascade(TwkDevice dev, int enable);
/* The merged layers the last such call kept: [layers][launchWidth*height] float4 — the explicit `layers` of twk_cascade_resolve
 * with width = launchWidth. TWK_ERROR_INVALID_STATE before such a call and after a drop. The read synchronises. */
int twk_get_temporal_cascade_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);
int twk_read_temporal_cascade(TwkDevice dev, float* host, size_t numFloats); /* numFloats = layers*launchWidth*height*4 */
/* Host only, no handle: the same definition over host arrays of the shapes above (4 floats per element). historyLayers NULL: every
 * pixel passes through. TWK_ERROR_INVALID_VALUE: as the explicit form. */
int twk_temporal_cascade_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                              const float* historyGeometry, const TwkCameraDefinition* historyCamera, int width, int height, float* layersOut);

/* ---- The rectified temporal merge — new calls, ABI stays 9, no existing struct changes; without them no kernel and no bit of any
 * existing call changes ---------------------------------------------------------------------------------------------------------
 * twk_update_light and twk_update_material leave the temporal history as it is, and twk_temporal_accumulate then keeps blending up
 * to maxHistory samples of the OLD lighting into every pixel; twk_temporal_reset is the only other remedy and throws the whole
 * picture's history away. twk_temporal_accumulate_rectified is twk_temporal_accumulate with a per-pixel TRUST t in [0, 1] in the
 * reprojected history: over a (2 radius + 1)^2 window of pixels of the same instance it tests the paired differences of the frame's
 * and the history's luminance means against their own scatter, and where the mean difference exceeds gamma standard errors it
 * scales the history's sample count (and M2) by t before the merge. The loop of "The temporal seam" with a light edit in it:
 *   twk_update_light(...);                                            (the history stays)
 *   twk_set_sample_offset; twk_launch 0 .. spp-1; twk_render_geometry; twk_temporal_accumulate_rectified;
 *   twk_denoise_variance_sampled(beauty = merged colour, moments = merged moments)
 * The complete definition, why it has this form and what it is not (luminance only; no re-traced temporal gradient; blind below the
 * window's noise; no colour clamp) is csrc/temporal_rectify_device.h; tests/temporal_rectify_restate.py restates it in numpy. Two
 * kernel launches and two f32 float4 scratch streams on the handle (allocated on first use, freed with the temporal history).
 * Where nothing is tested (t = 1) every output has the bits of twk_temporal_accumulate. The defaults are PROVISIONAL: they come
 * from a numpy prototype, not from a sweep on rendered frames (profiles/r22_temporal_rectify.md). */
typedef struct TwkTemporalRectify { int radius; int minTaps; float gamma; } TwkTemporalRectify;
#define TWK_TEMPORAL_RECTIFY_RADIUS 3
#define TWK_TEMPORAL_RECTIFY_MIN_TAPS 8
#define TWK_TEMPORAL_RECTIFY_GAMMA 3.0f
#define TWK_TEMPORAL_RECTIFY_MAX_RADIUS 4
int twk_temporal_rectify_defaults(TwkTemporalRectify* rp);
/* Both forms of twk_temporal_accumulate, with its arguments, its outputs and ALL its refusals, plus trustOut: width x height floats
 * (explicit form; may be NULL like the other outputs; must not overlap an input or another output), 1 where nothing was tested and
 * where there is no history, 0 where the test took all of a history that was there. Own-buffer form (current NULL: history, the
 * outputs and the size must be NULL / 0): the trust is kept on the handle (twk_get_temporal_trust_device_pointer,
 * twk_read_temporal_trust), the other results where twk_temporal_accumulate keeps them, and while twk_temporal_enable_cascade(1)
 * is set the layers are merged with the trust (twk_temporal_accumulate_cascade_trusted's definition). Plain and rectified calls
 * may alternate on one handle: they share the history. tp, rp NULL: the defaults. Asynchronous on the handle's stream.
 * Beside twk_temporal_accumulate's refusals, TWK_ERROR_INVALID_VALUE: radius outside 1..TWK_TEMPORAL_RECTIFY_MAX_RADIUS;
 * minTaps < 2; gamma negative or not finite. */
int twk_temporal_accumulate_rectified(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalRectify* rp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                                      int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut);
/* The trust plane of the last own-buffer (or assembled) rectified merge: one float per pixel of the temporal result.
 * TWK_ERROR_INVALID_STATE: the last own-buffer merge on the handle was not a rectified one, or its history has been dropped since. */
int twk_get_temporal_trust_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);
int twk_read_temporal_trust(TwkDevice dev, float* host, size_t numFloats);       /* width*height floats of the temporal result; synchronises */
/* twk_temporal_accumulate_cascade with a trust stream (width x height floats, a trustOut of the call above for the same frame and
 * history): after the cap, h[j] *= t, hrej *= t, hn *= t (csrc/temporal_cascade_device.h, "the TRUSTED build"). Same arguments,
 * same refusals; also TWK_ERROR_INVALID_VALUE for a NULL trust and for an output that overlaps it. */
int twk_temporal_accumulate_cascade_trusted(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                            const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, const void* trust,
                                            int width, int height, void* layersOut);
/* twk_temporal_accumulate_assembled with the rectified merge: on a tiled primary, the assembled planes as the current frame. Same
 * refusals as twk_temporal_accumulate_assembled, plus those of the parameters above. */
int twk_temporal_accumulate_assembled_rectified(TwkDevice primary, const TwkTemporal* tp, const TwkTemporalRectify* rp);
/* Pure CPU, no device: the definitions compiled for the host, for tests and for integrators without a GPU at hand. Host arrays of
 * width x height x 4 floats (trustOut: width x height); colour is RGBA32F (the merge's arithmetic does not depend on the output
 * format: narrow colourOut to get the RGBA16F result); history* all NULL or all given with historyCamera; outputs may be NULL. */
int twk_temporal_rectify_host(const TwkTemporal* tp, const TwkTemporalRectify* rp, const float* colour, const float* moments, const float* geometry,
                              const float* historyColour, const float* historyMoments, const float* historyGeometry, const TwkCameraDefinition* historyCamera,
                              int width, int height, float* colourOut, float* momentsOut, float* trustOut);
int twk_temporal_cascade_trusted_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                                      const float* historyGeometry, const TwkCameraDefinition* historyCamera, const float* trust, int width, int height, float* layersOut);

/* ---- Moving an object: the instance-transform update and motion in the temporal merges — new calls, ABI stays 9, no existing
 * struct, enum or constant changes; without them no kernel and no bit of any existing call changes --------------------------------
 * twk_update_instance_transform moves an instance and KEEPS the temporal history (twk_clear_scene + twk_build would drop it). The
 * merges then look the history up where the object was: a surface point of instance i now at world g was at
 * g' = M_prev,i . M_cur,i^-1 . g when the history was taken — one matrix per instance, TwkInstanceMotion. The own-buffer and the
 * assembled forms of twk_temporal_accumulate and twk_temporal_accumulate_rectified do this by themselves; the explicit forms with a
 * table are the *_moving calls below. The loop of "The temporal seam" with a moving object in it:
 *   twk_update_instance_transform(dev, id, M);                            (the history stays; the geometry AOV is stale)
 *   twk_set_sample_offset; twk_launch 0 .. spp-1; twk_render_geometry; twk_temporal_accumulate [_rectified];
 * The complete definition is csrc/temporal_motion_device.h; tests/temporal_motion_restate.py restates it in numpy. What it is not:
 * no deforming geometry here (vertex updates and per-vertex motion: "Deforming an object" below), no motion blur, no moving lights (an instance that carries a
 * light is refused), no environment reprojection, pinhole only. By default every update rebuilds the whole acceleration structure, as
 * twk_build does; "Selective instance updates" below rebuilds only what the moved instances change. Shadows and inter-reflections that the move changes ELSEWHERE are stale history like a
 * light edit's: the rectified merge discounts them.
 *
 * One record per instance, indexed by instance: previousFromCurrent is X = M_prev . M_cur^-1, row-major 3 x 4; moved = 0 says the
 * instance is where it was, and X (written as the identity) is never read. reserved: 0. */
typedef struct TwkInstanceMotion { float previousFromCurrent[12]; unsigned int moved; unsigned int reserved[3]; } TwkInstanceMotion; /* 64 bytes */
/* Pure CPU, no device. moved = 0 when the 24 words of previous and current are bit-equal; else X is computed in double from the
 * float inputs in a fixed operation order (the cofactor inverse of current, then the product row by row, left to right) and each
 * element is rounded to float once. TWK_ERROR_INVALID_VALUE: a NULL argument, an input that is not finite, a current whose 3 x 3
 * determinant is zero or not finite. */
int twk_instance_motion(const float previous[12], const float current[12], TwkInstanceMotion* out);
/* ≙ an OptiX instance-transform update followed by an IAS rebuild. Replaces the instance's object-to-world matrix (row-major 3 x 4,
 * as twk_add_instance takes it) and rebuilds the acceleration structure with the code of twk_build; synchronises, and
 * twk_get_build_info then describes this rebuild. After it the handle renders like a fresh handle built with the new transforms,
 * byte for byte; the geometry AOV is stale (twk_render_geometry first), adaptive state is dropped as twk_build drops it, and the
 * temporal history — colour, moments, geometry, camera, cascade layers, trust — is KEPT, together with the transforms of every
 * instance as of the frame the history was taken (refreshed when a merge swaps the history). Several updates may happen between
 * two merges. On several devices every handle is updated by the caller. TWK_ERROR_INVALID_STATE: before a successful twk_build.
 * TWK_ERROR_INVALID_VALUE: a NULL handle or transform (before any HIP call), an id out of range, a transform that is not finite or
 * whose 3 x 3 determinant is zero or not finite, and an instance with idLight >= 0 (the light definition holds the emitter's
 * position and would disagree; moving emitters is not supported). A rebuild that fails leaves the handle unbuilt, as twk_build does. */
int twk_update_instance_transform(TwkDevice dev, int idInstance, const float transform[12]);
/* The instance's transform as it is now. TWK_ERROR_INVALID_VALUE: a NULL argument, an id out of range. */
int twk_get_instance_transform(TwkDevice dev, int idInstance, float transform[12]);
/* ---- Selective instance updates — new calls, ABI stays 9; in the default mode every existing call launches what it launched ----
 * A handle built in TWK_UPDATE_SELECTIVE keeps the by-products of its build — the full-precision wide nodes (128 B per node), the
 * expected-visit cost per node (4 B, with costed cuts), the pair flags (4 B per triangle slot, with pairs) and, on the host, every
 * tree's box, height, SAH terms and leaf payload — and its transform updates rebuild only: the world-space tree of each moved
 * FLATTENED instance, at the node and slot range it already has; the top level; the 8-wide root; and the quantised copy and pair
 * references of exactly those node ranges, in one launch. A moved ENTERED instance changes its instance record and its box in the
 * top level; no bottom-level tree is ever rebuilt. Afterwards the handle equals, byte for byte, a fresh handle built with the
 * current transforms. Everything else about an update is as "Moving an object" says: the temporal history stays, adaptive state is
 * dropped, the geometry AOV is stale, and an update that fails (an allocation, a HIP error, the depth refusal, with twk_build's
 * text) leaves the handle unbuilt until twk_build. What it is not: not a refit (a moved flattened instance gets a new tree; twk_refit_instance_transform, "Refit of a moved instance" below, is the call that keeps the tree), no vertex
 * updates by these calls (twk_update_geometry_vertices: "Deforming an object" below), no adding or removing of instances, no change of flatten policy or build quality between updates (those need twk_build),
 * no moving emitters. Measured: profiles/r24_selective_update.md. */
#define TWK_UPDATE_FULL      0 /* default: an update rebuilds everything twk_build builds; nothing is kept */
#define TWK_UPDATE_SELECTIVE 1
/* The mode of the NEXT twk_build: a handle built in full mode keeps doing full updates until it is built again (TwkUpdateInfo.selective
 * says which ran). TWK_ERROR_INVALID_VALUE: a NULL handle (before any HIP call), any other mode. */
int twk_set_update_mode(TwkDevice dev, int mode);
/* Several moves, one rebuild: transforms holds 12 floats per entry. Works in both modes (full mode: one rebuild of everything for
 * count moves). Every refusal of twk_update_instance_transform applies per entry and names it ("entry k"); also
 * TWK_ERROR_INVALID_VALUE: count < 1, a NULL array, an id listed twice. A refused batch changes nothing.
 * twk_update_instance_transform is its count == 1 case. */
int twk_update_instance_transforms(TwkDevice dev, int count, const int* idInstances, const float* transforms);
/* What the last update did. selective: which path ran; treesRebuilt: world-space trees of moved flattened instances (full: every tree); nodesRequantised:
 * wide nodes the tail quantised (selective: the plan's total; full: all); slotsRewritten: triangle slots written; keptBytes: device
 * memory the selective mode keeps beyond a full-mode handle's (0 in full mode); milliseconds: host wall time of the update, also
 * TwkBuildInfo.buildMilliseconds. */
typedef struct TwkUpdateInfo
{
  int selective, instancesMoved, treesRebuilt, topLevelRebuilt;
  uint64_t nodesRequantised, slotsRewritten, instanceRecordsUploaded, keptBytes;
  double milliseconds;
} TwkUpdateInfo;
/* TWK_ERROR_INVALID_VALUE: a NULL argument. TWK_ERROR_INVALID_STATE: before the handle's first update, and after an update whose
 * rebuild failed (a refused update changes nothing and leaves the record of the update before it). */
int twk_get_update_info(TwkDevice dev, TwkUpdateInfo* info);
/* Pure CPU, no device: the plan of a selective update (csrc/update_plan.h, the code twk_build lays its scene out with). In:
 * instanceGeometry[numInstances], geometryTriangles[numGeometries], the flatten policy, maxLeaf (triangles per leaf, default 2; an
 * instance of no more triangles than that is a direct leaf of the top level) and the moved ids (numMoved may be 0: the layout
 * only). Out: plan; flattened[numInstances] (0/1) and trees[numMoved] (the flattened moved instances, ascending; plan->treesRebuilt
 * of them) and ranges[2 * (numMoved + 2)] ((first node, count) pairs; plan->numRanges of them: the rebuilt trees ascending, the top
 * level, the two root slots), each NULL or given. TWK_ERROR_INVALID_VALUE: NULL input or plan, counts < 1, a geometry index or moved
 * id out of range, a moved id listed twice, a negative triangle count. */
typedef struct TwkUpdatePlan
{
  int instances, flattenedInstances, directLeafInstances, enteredGeometries, treesRebuilt, topLevelRebuilt, numRanges, tlasBase;
  uint64_t nodes, triangleSlots, nodesRequantised, slotsRewritten;
} TwkUpdatePlan;
int twk_update_plan_host(const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries, int flattenMaxTriangles,
                         int flattenMaxReferences, int maxLeaf, const int* moved, int numMoved, TwkUpdatePlan* plan, unsigned char* flattened, int* trees, int* ranges);
/* ---- Deforming an object: the vertex update and the previous-position plane — new calls, ABI stays 9, no existing struct, enum or
 * constant changes; while no vertex update has been made every existing call launches the kernels it launched --------------------
 * twk_update_geometry_vertices replaces the vertices of one geometry (≙ rebuilding an OptiX GAS on a new vertex buffer, which the
 * reference's Device::createGeometry cannot do) and KEEPS the temporal history; twk_render_geometry_motion then says, per pixel,
 * where the surface point it sees was when the history was taken. The complete definition of that plane is
 * csrc/temporal_carry_device.h; tests/temporal_carry_restate.py restates it in numpy. What it is not: no topology change (the indices
 * stay), not a refit (a changed tree is rebuilt, or the equality below would not hold; twk_refit_geometry_vertices, "Refit" below, is the call that keeps the topology), no device-pointer source for the vertices in THIS call (twk_update_geometry_vertices_device, "A device-pointer source" below, takes one), no
 * emitting geometry, no motion blur, no tiled frames (the assembled forms refuse while a geometry is deformed), pinhole only, no
 * rtigo3_hip key. The merges read the plane through their Carried builds, further below. Measured: profiles/r25_vertex_update.md (tools/vertex_update_time.py).
 *
 * Replaces all TwkTriangleAttributes of geometry idGeometry (positions, tangents, normals, texcoords; the caller keeps them
 * consistent); the indices, and so topology and triangle pairing, stay. Rebuilds the acceleration structure and synchronises;
 * twk_get_build_info then describes this rebuild. Afterwards the handle equals, byte for byte, a fresh handle that was given the new
 * vertices through twk_clear_scene ... twk_build: acceleration structure, scene arrays, build info except its time, every picture.
 * A handle built in full mode rebuilds everything; one built in TWK_UPDATE_SELECTIVE uploads the geometry's attributes and rebuilds
 * the bottom-level tree of the geometry at the node and slot range it has (if some instance enters it — the first bottom-level tree
 * the selective path rebuilds), the world box of every entered instance of it, the world-space tree of every flattened instance of
 * it, the top level, the 8-wide root, and the quantised copy and pair references of exactly those ranges. twk_get_update_info
 * describes it: instancesMoved 0, treesRebuilt = the bottom-level tree, if any, plus the flattened trees, instanceRecordsUploaded 0.
 * As for a transform update the temporal history is kept, adaptive state is dropped and the geometry AOV is stale.
 * The first update of a geometry since the history's frame keeps the geometry's object-space positions as of that frame (several
 * updates between two merges keep the oldest): the geometry is DEFORMED (twk_get_geometry_deformed) until an own-buffer merge swaps
 * the history or twk_temporal_reset, twk_build or twk_clear_scene drop it. Without a history nothing is kept.
 * A refused call changes nothing; a rebuild that fails leaves the handle unbuilt, as twk_build does. TWK_ERROR_INVALID_VALUE: a NULL
 * handle or array (before any HIP call), an id out of range, numAttributes different from the geometry's vertex count, a position
 * that is not finite, a geometry that an instance with idLight >= 0 references (the light definition holds the emitter's shape and
 * would disagree). TWK_ERROR_INVALID_STATE: before a successful twk_build. */
int twk_update_geometry_vertices(TwkDevice dev, int idGeometry, const TwkTriangleAttributes* attributes, size_t numAttributes);
/* Whether the handle holds previous positions of the geometry (above). TWK_ERROR_INVALID_VALUE: a NULL argument, an id out of range. */
int twk_get_geometry_deformed(TwkDevice dev, int idGeometry, int* deformed);
/* twk_update_plan_host with updated geometries as well as moved instances (either count may be 0): the plan of
 * twk_update_geometry_vertices is the one with numMoved 0 and the one geometry. plan->treesRebuilt counts the bottom-level trees of
 * the updated geometries that some instance enters and the world-space trees of the flattened instances among the moved ones and
 * among the instances of the updated geometries; trees[] lists them, a bottom-level tree as ~geometry (negative) first, and ranges[]
 * their node ranges in the same order (ascending and disjoint), then the top level and the two root slots: give both room for
 * numGeometries + numInstances + 2 entries. Refusals as twk_update_plan_host's, plus an updated id out of range or listed twice. */
int twk_vertex_update_plan_host(const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries, int flattenMaxTriangles,
                                int flattenMaxReferences, int maxLeaf, const int* moved, int numMoved, const int* updatedGeometries, int numUpdated,
                                TwkUpdatePlan* plan, unsigned char* flattened, int* trees, int* ranges);
/* ---- Refit: a deformed mesh's trees updated in place — new calls, ABI stays 9; the full and the selective mode launch what they
 * launched -------------------------------------------------------------------------------------------------------------------------
 * twk_refit_geometry_vertices is twk_update_geometry_vertices for a handle built in TWK_UPDATE_SELECTIVE (≙ an OptiX build with
 * OPTIX_BUILD_OPERATION_UPDATE): the same arguments, the same refusals with the same texts under its own name, the same treatment
 * of everything around the trees — the previous positions are kept (the geometry counts as deformed), the temporal history stays,
 * adaptive state is dropped, the geometry AOV is stale, twk_get_build_info and twk_get_update_info (selective 1, treesRebuilt = the
 * trees really rebuilt) describe the call. But the bottom-level tree of the geometry (if some instance enters it) and the world-space
 * tree of every flattened instance of it are REFIT, not rebuilt (csrc/bvh_refit.h is the complete definition): every slot and shading
 * record is written again from the primitive word the slot holds, every leaf box follows the build's rule (padBox once per build
 * primitive), every inner box is the union of its children's, every wide node keeps the cut it had, and the node costs follow. The
 * references, the slot order, the pair flags and the heights do not change. A direct-leaf instance (no tree of its own) takes the
 * rebuild's path and counts in treesRebuilt. All refit trees of the call go through ONE launch sequence with ONE host wait
 * (csrc/bvh_refit.hip, the one batch every refit call runs; csrc/refit_scene_plan.h says which trees and of which kind). The top
 * level, the 8-wide root and the ranged tail run as in the selective update.
 * The result is a LEGAL tree for the new vertices (tests/bvh_audit.py holds it to every check a build's tree passes), not the tree a
 * fresh build would choose: its quality decays as the mesh moves away from the vertices it was built from. TwkRefitInfo says by how
 * much — sahNow / sahBuilt — and the caller decides when to call twk_update_geometry_vertices, which rebuilds: there is no fallback
 * in the library. A refit with the vertices the tree was built from changes no byte; a refit back to them restores every byte.
 * What it is not: no refit of a MOVED flattened instance by THIS call (twk_refit_instance_transform, "Refit of a moved instance" below, is that call), no restructuring or rotations, no new
 * cuts, no topology change, no emitters, no tiled frames while a geometry is deformed, no device-pointer source in this call (twk_refit_geometry_vertices_device takes one), no rtigo3_hip key.
 * Additional refusal: TWK_ERROR_INVALID_STATE on a handle whose scene was not built in TWK_UPDATE_SELECTIVE (twk_set_update_mode
 * before twk_build): nothing a refit needs was kept. Measured: profiles/r28_refit.md (tools/refit_time.py). */
int twk_refit_geometry_vertices(TwkDevice dev, int idGeometry, const TwkTriangleAttributes* attributes, size_t numAttributes);
/* What the last refit did. treesRefit / treesRebuilt: trees refit in place / rebuilt (direct-leaf instances); nodesRefit: nodes of
 * the refit trees' ranges; slotsRewritten: triangle slots written; sahBuilt: the sum of sahInner + sahLeaf of the refit trees as of
 * their last real build (twk_build, twk_update_geometry_vertices, a transform update of a flattened instance — each resets the
 * tree's count and its sahBuilt); sahNow: the same sum after this refit; refitsSinceBuild: the largest number of refits any of the
 * refit trees has taken since it was last built; milliseconds: host wall time, also TwkBuildInfo.buildMilliseconds. */
typedef struct TwkRefitInfo
{
  int treesRefit, treesRebuilt, topLevelRebuilt, refitsSinceBuild;
  uint64_t nodesRefit, slotsRewritten;
  double sahBuilt, sahNow, milliseconds;
} TwkRefitInfo;
/* TWK_ERROR_INVALID_VALUE: a NULL argument. TWK_ERROR_INVALID_STATE: no refit has been made on this handle since it was last built. */
int twk_get_refit_info(TwkDevice dev, TwkRefitInfo* info);
/* Pure CPU, no device: the refit of ONE tree from host arrays, with the header's code. All arrays are the TREE's own: nodes
 * [numNodes x 16 floats] binary nodes and wideNodes [numNodes x 32 floats] full-precision wide nodes (in / out), nodeCost [numNodes]
 * (in / out, or NULL: the cuts were not costed), slots [numSlots x 12 floats] (in: the primitive word of each slot; out: the
 * vertices) and shadeRecords [numSlots x 32 floats] (out), pairFlags [numSlots] (or NULL), the geometry's attributes and indices
 * (numIndices = 3 x numSlots). References in the nodes are absolute: node nodeBase + i stands at nodes[16 i], slot slotBase + s at
 * slots[12 s]. leafFlag 0: an object-space tree (transform ignored); TWK_LEAF_WORLD (0x40000000): the world-space tree of instance
 * idInstance under `transform` (row-major 3 x 4), whose slots get the instance word. terms[2] (or NULL): sahInner, sahLeaf;
 * rootBounds[6] (or NULL): the tree's box. TWK_ERROR_INVALID_VALUE: a NULL array, a count < 1 or out of range, numIndices different
 * from 3 x numSlots, an index beyond the attributes, a leafFlag that is neither, a world-space tree without transform or with a
 * negative instance, a reference that leaves the ranges given or names a node twice, a primitive word beyond the indices. */
int twk_refit_tree_host(float* nodes, float* wideNodes, float* nodeCost, float* slots, float* shadeRecords, const int* pairFlags,
                        const TwkTriangleAttributes* attributes, size_t numAttributes, const unsigned int* indices, size_t numIndices,
                        int nodeBase, int numNodes, int slotBase, int numSlots, int leafFlag, const float* transform, int idInstance,
                        double* terms, float* rootBounds);
/* The three device arrays a selective handle keeps, for comparing the device with the host form: wide [32 x (nodes + 2) floats]
 * (the full-precision wide nodes and the two root slots), nodeCost [nodes floats], pairFlags [triangleSlots ints]; each NULL or
 * given with its count of elements. TWK_ERROR_INVALID_STATE: the handle is not built in TWK_UPDATE_SELECTIVE, or does not keep an
 * array that is asked for (no costed cuts, no pairs). TWK_ERROR_INVALID_VALUE: a NULL handle, a count that is not the array's. */
int twk_debug_read_kept_build(TwkDevice dev, float* wide, size_t numWideFloats, float* nodeCost, size_t numNodeCost, int* pairFlags, size_t numPairFlags);
/* ---- Refit of a moved instance: a dragged object without a tree build — new calls, ABI stays 9; every existing call launches what
 * it launched ----------------------------------------------------------------------------------------------------------------------
 * twk_refit_instance_transform[s] are twk_update_instance_transform[s] for a handle built in TWK_UPDATE_SELECTIVE: the same
 * arguments, the same refusals in the same order with the same texts under their own names (a NULL handle or array before any HIP
 * call, before twk_build, a bad id, a transform that is not finite or singular, an instance that carries a light, an id listed
 * twice, count < 1; a refused batch changes nothing), and the same treatment of everything around the trees: the temporal history
 * and the transforms as of its frame are kept — twk_read_temporal_motion and the merges work afterwards unchanged — adaptive state is
 * dropped, the geometry AOV is stale. What each moved instance gets: an ENTERED one its world box in the top level, as in the
 * selective update; a DIRECT-LEAF one (two triangles, a leaf of the top level itself) the rebuild's path, counted in treesRebuilt;
 * every other FLATTENED one a REFIT IN PLACE of its world-space tree: every slot is written again from the primitive word it holds,
 * through the new matrix, with the build's expression; every leaf box, inner box, wide node (with the cut it had) and node cost
 * follows as csrc/bvh_refit.h defines; the SAH terms follow. The 128-byte shading records are not touched: they are object-space,
 * and a transform does not change them. All trees of a call are refit by ONE launch sequence with ONE host wait
 * (csrc/bvh_refit.hip, the one batch every refit call runs; csrc/refit_batch_plan.h plans its blocks). Then the top level, the depth check, the 8-wide root, the ranged
 * tail, the top caches, as in the selective update. twk_get_update_info (selective 1, instancesMoved = count, treesRebuilt = the
 * direct leaves) and twk_get_refit_info describe the call; each refit tree's count of refits goes up by one.
 * The result is a LEGAL scene for the new transforms, not a fresh build's. For a translation or a uniform scale the refit tree is
 * the tree a rebuild would choose, moved; under a rotation or an unequal scale its boxes grow looser than a rebuild's, and
 * TwkRefitInfo.sahNow / sahBuilt says by how much: the caller decides when to call twk_update_instance_transform, which rebuilds
 * the tree and resets its count. There is no fallback in the library. A refit with the transforms the scene was built with changes
 * no byte; a refit back to them restores every byte.
 * What it is not: no restructuring, no new cuts, no automatic refit-or-rebuild choice, no moving emitters, no rtigo3_hip key; on a
 * tiled frame every handle is moved by the same call, as for twk_update_instance_transform.
 * Additional refusal, after "before twk_build": TWK_ERROR_INVALID_STATE on a handle whose scene was not built in
 * TWK_UPDATE_SELECTIVE. Measured: profiles/r31_instance_refit.md (tools/instance_refit_time.py). */
int twk_refit_instance_transform(TwkDevice dev, int idInstance, const float transform[12]);
int twk_refit_instance_transforms(TwkDevice dev, int count, const int* idInstances, const float* transforms);
/* Pure CPU, no device: how the trees of one batched refit share its launches (csrc/refit_batch_plan.h, the code the call plans
 * with). Tree k has treeNodes[k] nodes and treeSlots[k] slots and occupies ceil(n / 256) consecutive node blocks and ceil(s / 256)
 * consecutive slot blocks, so that no block straddles two trees. Out, each NULL or given: nodeOffsets / slotOffsets [numTrees] (the
 * nodes / slots of the trees before it; at the node offset stand its parents and tickets), nodeBlockFirst /
 * slotBlockFirst [numTrees] (its first block: where its partial sums stand), nodeBlocks [2 x plan->nodeBlocks] / slotBlocks
 * [2 x plan->slotBlocks] (per block: its tree, the tree-local index of its first thread). The block counts are those sums of
 * ceilings (or call once with the tables NULL). TWK_ERROR_INVALID_VALUE: a NULL input or plan, numTrees < 1, a tree with less than
 * one node or slot, 2^31 or more nodes, slots or threads in all. */
typedef struct TwkRefitBatchPlan
{
  int trees, nodeBlocks, slotBlocks, blockThreads;
  uint64_t nodes, slots;
} TwkRefitBatchPlan;
int twk_refit_batch_plan_host(const int* treeNodes, const int* treeSlots, int numTrees, TwkRefitBatchPlan* plan, int* nodeOffsets, int* slotOffsets,
                              int* nodeBlockFirst, int* slotBlockFirst, int* nodeBlocks, int* slotBlocks);
/* ---- A device-pointer source for the vertices — new calls, ABI stays 9; every existing call launches what it launched ------------
 * twk_update_geometry_vertices_device and twk_refit_geometry_vertices_device are the two calls above for vertices that already live
 * on the device (skinning, cloth, a simulation step, a torch tensor; ≙ OptixBuildInputTriangleArray::vertexBuffers, a device pointer
 * with vertexStrideInBytes): no copy to the host, no host loop over the vertices, no upload. csrc/vertex_source_device.h is the
 * complete definition; tests/vertex_source_restate.py restates the frames in numpy.
 * The source is ONE of: attributes — numVertices TwkTriangleAttributes records, 16-byte aligned; positions — x, y, z floats per
 * vertex, positionStride bytes apart (0 means 12), 4-byte aligned, with recomputeFrames 0 (tangents and normals stay) or 1 (they
 * follow the new positions: the area-weighted sum of the adjacent triangles' normals in a fixed order, the tangent made
 * perpendicular to it; an unusable sum keeps the old vector; texture coordinates always stay).
 * THE CONTRACT: after the call the handle equals, byte for byte, a handle that was given the same records through the host call of
 * the same name — acceleration structure, scene arrays, TwkBuildInfo / TwkUpdateInfo / TwkRefitInfo apart from the millisecond
 * fields, every picture, the previous-position plane. "The same records": in attributes mode the source read back; in positions
 * mode twk_vertex_frames_host(positions, ..., before = the geometry's records before the call), and with recomputeFrames 0 those
 * `before` records with vertex[] replaced. twk_read_geometry_vertices returns them.
 * STREAM RULE: the source is read on the handle's stream. The caller must have finished producing it — by synchronising its own
 * stream or waiting on its event — before the call; on return the source has been consumed and may be overwritten.
 * What it is not: no welding, no angle weights, no creases, no skinning (no bones, no weights), no index or topology change, no
 * emitters, no asynchronous refit (the call's own waits stay), no tiled frames while a geometry is deformed, no rtigo3_hip key.
 * Refusals, all under the call's own name, after which nothing has changed: every refusal of the host call of the same name (a NULL
 * handle, before twk_build, a refit on a handle not built in TWK_UPDATE_SELECTIVE, a bad id, a wrong vertex count, a geometry with
 * an instance that carries a light); TWK_ERROR_INVALID_VALUE: a NULL source, both pointers or neither, a stride below 12 or no
 * multiple of 4 (or any with attributes), recomputeFrames above 1 (or 1 with attributes), a reserved word that is not 0, a
 * misaligned pointer, a pointer that hipPointerGetAttributes does not report as device or managed memory the handle's device can
 * read (a plain host pointer: nothing is dereferenced), an allocation that ends before the last vertex, a source that overlaps the
 * handle's own attribute array, and a position that is not finite — "vertex <lowest such index>: the position is not finite", found
 * by a read-only launch before anything is written. Measured: profiles/r29_vertex_source.md (tools/vertex_source_time.py). */
typedef struct TwkVertexSource
{
  const void* attributes;       /* device pointer to numVertices TwkTriangleAttributes (48 B each), or NULL */
  const void* positions;        /* device pointer to x,y,z floats per vertex, or NULL; exactly one of the two is set */
  size_t      positionStride;   /* bytes between two positions: >= 12, a multiple of 4; 0 means 12 */
  unsigned    recomputeFrames;  /* positions mode only: 1 = normals and tangents from the new positions, 0 = keep them */
  unsigned    reserved[3];      /* must be 0 */
} TwkVertexSource;
int twk_update_geometry_vertices_device(TwkDevice dev, int idGeometry, const TwkVertexSource* source, size_t numVertices);
int twk_refit_geometry_vertices_device(TwkDevice dev, int idGeometry, const TwkVertexSource* source, size_t numVertices);
/* Pure CPU, no device: the records of a positions-mode source with recomputeFrames 1, with the code the kernel runs. positions:
 * three floats per vertex; before / after: numVertices records (they may be the same array). TWK_ERROR_INVALID_VALUE: a NULL
 * argument, numVertices 0, numIndices 0 or no multiple of three, an index beyond the vertices. */
int twk_vertex_frames_host(const float* positions, size_t numVertices, const unsigned int* indices, size_t numIndices,
                           const TwkTriangleAttributes* before, TwkTriangleAttributes* after);
/* The geometry's current records, wherever they were last written (a device-pointer source leaves them on the device: one copy
 * back). capacity: records `out` has room for. TWK_ERROR_INVALID_VALUE: a NULL argument, a bad id, a capacity below the count. */
int twk_read_geometry_vertices(TwkDevice dev, int idGeometry, TwkTriangleAttributes* out, size_t capacity);
/* ---- A frame's edits in one call: deformed meshes and moved instances — new calls, ABI stays 9; every existing call launches what
 * it launched ----------------------------------------------------------------------------------------------------------------------
 * twk_refit_scene takes what a frame edits — numGeometries geometries with new vertices, each from host records (attributes) or from
 * a device source (source; "A device-pointer source" above), and numInstances instances with new transforms — and refits the handle
 * ONCE. THE SEQUENCE it stands for: twk_refit_geometry_vertices or twk_refit_geometry_vertices_device for every geometry entry in
 * the order given, then twk_refit_instance_transforms for the instances. After twk_refit_scene the handle holds, byte for byte, what
 * the sequence leaves: binary and quantised nodes, slots, shading records, instance records, both top-level caches, the kept arrays
 * (twk_debug_read_kept_build), the attribute array (twk_read_geometry_vertices), twk_get_instance_transform, the previous positions
 * and the transform snapshot of the temporal history, every picture — a refit tree is a function of its topology, the vertices and
 * the matrix alone. What differs is the bookkeeping: every tree is refit once, so its count of refits goes up by ONE (also the tree
 * of an instance that is both moved and of an edited geometry), and TwkRefitInfo / TwkUpdateInfo describe the one call — treesRefit,
 * nodesRefit, sahBuilt and sahNow count each refit tree once, treesRebuilt the direct-leaf instances (the rebuild's path, as in the
 * calls above), slotsRewritten the slots of all those trees, instancesMoved = numInstances. (TwkUpdateInfo.keptBytes equals the
 * sequence's: no refit call writes soup descriptors for a refit tree, so none grows that scratch.)
 * Each instance gets what its kind needs: a moved or edited ENTERED one its world box (from its geometry's new root box where that
 * was refit in this call), a DIRECT LEAF the rebuild, every other FLATTENED one a refit in place. All refit trees — bottom-level
 * trees of edited geometries, world-space trees of instances of edited geometries, world-space trees of moved instances — go through
 * ONE upload, five launches, one read-back and ONE host wait, whatever their number and kinds (csrc/bvh_refit.hip, the batch the
 * single refit calls run too; csrc/refit_scene_plan.h says which tree is of which kind): the slot kernel makes every soup descriptor in registers, so no
 * descriptor launch runs per tree. All device sources are checked before anything is written: one check launch per source into one
 * result array, ONE read-back and wait, then the ingest launches. The stages around the trees (top level, depth check, 8-wide root,
 * ranged tail, top caches) run once, as in the selective update. numGeometries == 0 makes the call twk_refit_instance_transforms;
 * numInstances == 0 with one entry makes it the vertex refit.
 * STREAM RULE: as for a device-pointer source — every source is read on the handle's stream, must have been produced before the
 * call, and has been consumed on return.
 * What it is not: no rebuilding counterpart, no asynchronous form (the batch's wait and the selective update's own waits stay), no
 * emitters, no topology change, no restructuring or new cuts, no automatic refit-or-rebuild choice, no tiled frames while a geometry
 * is deformed, no rtigo3_hip key; the four refit calls above keep their own launches.
 * Refusals, all under the name twk_refit_scene, in this order, after which nothing has changed:
 *  1. TWK_ERROR_INVALID_VALUE: a negative count, both counts 0, a NULL array with a positive count;
 *  2. a NULL handle; TWK_ERROR_INVALID_STATE: before twk_build, a handle not built in TWK_UPDATE_SELECTIVE;
 *  3. per geometry entry in order, "geometry entry k: " in front: neither or both of attributes and source, reserved not 0, a
 *     geometry listed twice; then the texts of twk_refit_geometry_vertices for a host entry (a bad id, a wrong vertex count, a
 *     position that is not finite, an instance of the geometry that carries a light) or of twk_refit_geometry_vertices_device for a
 *     device entry (those, and the source's own: both pointers or neither, a reserved word, recomputeFrames, the stride, the
 *     alignment, memory the device cannot read, an allocation that ends early, an overlap with the handle's attribute array);
 *  4. per instance entry, "entry k: " in front, the texts of twk_refit_instance_transforms (a bad id, a transform that is not finite
 *     or singular, an instance that carries a light, an id listed twice);
 *  5. last, a device source with a position that is not finite: "geometry entry k: vertex v: the position is not finite", k the
 *     lowest such entry and v its lowest such vertex.
 * Measured: profiles/r32_scene_refit.md (tools/scene_refit_time.py). */
typedef struct TwkGeometryEdit
{
  int32_t  idGeometry;
  uint32_t reserved;                        /* 0 */
  uint64_t numVertices;
  const TwkTriangleAttributes* attributes;  /* host records, or NULL */
  const TwkVertexSource*       source;      /* device source, or NULL; exactly one of the two */
} TwkGeometryEdit;                          /* 32 bytes */
int twk_refit_scene(TwkDevice dev, int numGeometries, const TwkGeometryEdit* geometries, int numInstances, const int* idInstances, const float* transforms);
/* Pure CPU, no device: the batch of a twk_refit_scene call on a scene laid out as twk_vertex_update_plan_host lays it out
 * (csrc/refit_scene_plan.h, the code the call plans with), for the instances `moved` and the geometries `updatedGeometries`. The
 * trees in batch order: the bottom-level trees of the updated entered geometries, ascending, listed as ~geometry, then the plan's
 * flattened instances that are no direct leaves, ascending. Out, each NULL or given, [plan->trees] (at most numGeometries +
 * numInstances): trees, kinds (0: bottom-level tree of an edited geometry, 176 bytes written per slot; 1: world-space tree of an
 * instance of an edited geometry, 176; 2: world-space tree of a moved instance of an unedited geometry, 48), nodeBases / nodeCounts /
 * slotBases / slotCounts (its ranges in the scene's arrays), and twk_refit_batch_plan_host's tables for those trees: nodeOffsets,
 * slotOffsets, nodeBlockFirst, slotBlockFirst, nodeBlocks [2 x plan->nodeBlocks], slotBlocks [2 x plan->slotBlocks] (call once with
 * the tables NULL for the counts). plan: the totals — directLeaves: instances that take the rebuild's path; boxes: entered instances
 * whose world box is written; slotsRewritten: the slots of the batch and of the direct leaves; slotBytes: bytes the slot kernel
 * writes. Refusals: twk_vertex_update_plan_host's, and 2^31 or more nodes, slots or threads in the batch. */
typedef struct TwkSceneRefitPlan
{
  int trees, nodeBlocks, slotBlocks, blockThreads;
  int directLeaves, boxes, topLevelRebuilt, reserved;
  uint64_t nodes, slots, slotsRewritten, slotBytes;
} TwkSceneRefitPlan;
int twk_scene_refit_plan_host(const int* instanceGeometry, int numInstances, const int* geometryTriangles, int numGeometries, int flattenMaxTriangles,
                              int flattenMaxReferences, int maxLeaf, const int* moved, int numMoved, const int* updatedGeometries, int numUpdated,
                              TwkSceneRefitPlan* plan, int* trees, int* kinds, int* nodeBases, int* nodeCounts, int* slotBases, int* slotCounts,
                              int* nodeOffsets, int* slotOffsets, int* nodeBlockFirst, int* slotBlockFirst, int* nodeBlocks, int* slotBlocks);
/* ---- Moving a light: emitters through the transform calls — new calls and an opt-in switch, ABI stays 9; no kernel changes --------
 * twk_enable_emitter_motion(dev, 1) makes the five transform entries — twk_update_instance_transform[s],
 * twk_refit_instance_transform[s] and the instance list of twk_refit_scene — accept an instance that carries a light (idLight >= 0)
 * and carry the light's definition along: the call sets the transforms as always, sets the light's definition to the one derived
 * below, uploads that one 80-byte record on the handle's stream, and then rebuilds, updates or refits exactly as for any other
 * instance (the light quad is an ordinary two-triangle instance). With the switch at its default 0 every call refuses such an
 * instance with the text it always had. twk_get_emitter_motion reads the switch, twk_get_light the definition as it is now.
 * THE RULE (csrc/light_motion.h is the complete definition; tests/light_motion_restate.py restates it in numpy): a light's ANCHOR is
 * the pair (its definition, its instance's transform) at the moment an emitter of that light is first moved. Every moved definition
 * is derived from the anchor, never from the one before it: a transform with the anchor transform's 48 bytes gives back the anchor
 * definition's 80 bytes (A -> B -> A is exact); otherwise D = T_new . inv(T_anchor) in double (the inverse and summation order of
 * twk_instance_motion, D not rounded), position = (float)(D p0), vecU = (float)(D_lin U0), vecV = (float)(D_lin V0), then in float
 * n = cross(vecU, vecV), area = |n|, normal = n / area (≙ createLights, reference Application.cpp:616-618), and normal is negated
 * when det(D_lin) < 0 — the emitter's lit side follows the inverse transpose, which a mirror does not flip, cross(vecU, vecV) does.
 * type, emission and the unused words are copied. twk_update_light on the light drops its anchor: the next move anchors on the new
 * definition and the transform of that moment. twk_init_lights, twk_build and twk_clear_scene drop every anchor.
 * THE CONTRACT: after an accepted call the handle equals, byte for byte, a fresh handle built with the new transform and
 * twk_get_light's definition (for the refit calls: the refit contract of twk_refit_instance_transform instead of the acceleration
 * structure's bytes). The temporal history stays, and its transform snapshot covers the emitter like every instance: the merges
 * follow the emitter's own pixels through the motion table; what the moved light changes elsewhere is stale history like any light
 * edit (twk_temporal_accumulate_rectified discounts it).
 * What it is not: no deforming or re-meshing of an emitter (the vertex calls keep refusing an emitting geometry), no moving
 * environment light, no light carried by several instances, no shape but the parallelogram, not on by default, and no guarantee that
 * the caller's definition matched the quad in the first place — the rule moves whatever definition it was given.
 * Refusals with the switch on, all TWK_ERROR_INVALID_VALUE under the call's name ("entry k: " in front in the batch forms), after
 * every refusal the call had before, in entry order, and before anything is changed: the light is not a TWK_LIGHT_PARALLELOGRAM;
 * the light is carried by more than one instance (the text names both); the derived area is zero or not finite, or a derived
 * component is not finite. twk_enable_emitter_motion: a NULL handle, a switch that is neither 0 nor 1. twk_get_emitter_motion,
 * twk_get_light: a NULL argument, a bad light id. Measured: profiles/r33_emitter_motion.md (tools/emitter_motion_time.py). */
int twk_enable_emitter_motion(TwkDevice dev, int on);
int twk_get_emitter_motion(TwkDevice dev, int* on);
int twk_get_light(TwkDevice dev, int idLight, TwkLightDefinition* out);
/* Pure CPU, no device, no HIP call: the rule above — `out` is `anchor` moved from anchorTransform to transform (row-major 3 x 4
 * object-to-world matrices; out may be anchor). TWK_ERROR_INVALID_VALUE: a NULL argument, an anchor that is no
 * TWK_LIGHT_PARALLELOGRAM, a transform that is not finite or an anchor transform whose 3 x 3 determinant is zero or not finite, a
 * derived area that is zero or not finite or a derived component that is not finite; `out` is then untouched. */
int twk_light_moved_host(const TwkLightDefinition* anchor, const float anchorTransform[12], const float transform[12], TwkLightDefinition* out);
/* One record per instance beside its TwkInstanceMotion (csrc/temporal_carry_device.h): previousObjectToWorld is the instance's
 * object-to-world matrix as of the history's frame, row-major 3 x 4; deformed = 0 says its geometry holds no previous positions and
 * nothing else is read; positionBase / indexBase: the first previous position / first index of its geometry in the arrays given. */
typedef struct TwkInstanceCarry { float previousObjectToWorld[12]; unsigned int deformed, positionBase, indexBase, reserved; } TwkInstanceCarry; /* 64 bytes */
/* twk_render_geometry with a second plane: one launch of a kernel of its own (picture-shaped handles only) writes the geometry AOV
 * exactly as twk_render_geometry does and, beside it, one float4 per pixel, always f32: a miss (0, 0, 0, bits 0); a hit
 * (g'.xyz, bits of g.w), where g' is where the surface point was when the history was taken — on a deformed geometry the hit's
 * barycentrics on the triangle's previous vertices through the instance's object-to-world matrix of that frame, on an instance that
 * has only moved X g of TwkInstanceMotion (the same bits), else g itself. Without a history, and after a merge has swapped it, every
 * hit's g' is g. The plane goes stale with the geometry AOV and when a merge swaps the history. Refusals: those of
 * twk_render_geometry, with its texts (a packed tile buffer included); TWK_ERROR_INVALID_VALUE: a NULL handle. */
int twk_render_geometry_motion(TwkDevice dev);
/* The plane: width x height float4. TWK_ERROR_INVALID_STATE: no valid plane (twk_render_geometry_motion first). */
int twk_get_previous_position_device_pointer(TwkDevice dev, void** dptr, size_t* bytes);
int twk_read_previous_positions(TwkDevice dev, float* host, size_t numFloats);
/* Pure CPU, no device: the plane of numPixels pixels from host arrays with the code the kernel runs. hits: (t, beta, gamma) per
 * pixel; instance (< 0: a miss) and primitive (local to the geometry) per pixel; geometry: the geometry AOV, four floats per pixel;
 * indices[numIndices]; previousPositions: four floats per vertex, numPositions of them; motion[numMotion] and carry[numCarry],
 * indexed by instance (an instance beyond a table is unmoved / not deformed); plane: four floats per pixel.
 * TWK_ERROR_INVALID_VALUE: a NULL argument, numPixels outside 1..2^28, a negative count or a count without its array, a deformed
 * hit whose primitive or vertices lie beyond the arrays given. */
int twk_previous_positions_host(const float* hits, const int* instance, const int* primitive, const float* geometry, size_t numPixels, const unsigned int* indices, size_t numIndices,
                                const float* previousPositions, size_t numPositions, const TwkInstanceMotion* motion, int numMotion, const TwkInstanceCarry* carry, int numCarry, float* plane);
/* The merges read the plane: the Carried builds (csrc/temporal_carry_device.h temporalCarry). Per candidate pixel p,
 * gp = previousPositions[p]; there is no history unless bits(gp.w) == bits(g.w) and gp.xyz is finite; everything after that is the
 * existing merge — the projection of gp, the taps' position test against gp, the cap, the blend, the trust. One more coalesced
 * 16-byte read per pixel, no table (the plane holds X g of a moved instance already); kernels of their own.
 * OWN-BUFFER forms (twk_temporal_accumulate, twk_temporal_accumulate_rectified and the cascade merge they drive): while no geometry
 * is deformed they do exactly what they did — the table, or nothing. While one is deformed they need a valid plane and otherwise
 * refuse with TWK_ERROR_INVALID_STATE ("... twk_render_geometry_motion first"); with it they launch the Carried builds, and
 * twk_read_temporal_motion then reports no table. On a tiled frame twk_temporal_accumulate_assembled[_rectified] and
 * twk_assemble_devices_with_geometry refuse while a geometry is deformed on the primary handle (TWK_ERROR_INVALID_STATE).
 * EXPLICIT forms: the arguments of twk_temporal_accumulate_moving / twk_temporal_accumulate_cascade_moving with previousPositions
 * (a DEVICE pointer to width x height float4, 16-byte aligned) in place of the table; rp NULL: the plain merge (trustOut must be
 * NULL), rp given: the rectified one; trust NULL: the cascade's plain merge, given: the trusted one. previousPositions NULL, or no
 * history, launches the existing kernels: byte for byte the existing call. Every refusal of those calls applies; also
 * TWK_ERROR_INVALID_VALUE: previousPositions not 16-byte aligned, an output overlapping it. */
int twk_temporal_accumulate_carried(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalRectify* rp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                                    const void* previousPositions, int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut);
int twk_temporal_accumulate_cascade_carried(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                            const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, const void* trust,
                                            const void* previousPositions, int width, int height, void* layersOut);
/* Pure CPU, no device: twk_temporal_moving_host / twk_temporal_cascade_moving_host with the plane (host, four floats per pixel) in
 * place of the table, the same headers compiled for the host. previousPositions NULL: the existing host forms. Refusals as theirs. */
int twk_temporal_carried_host(const TwkTemporal* tp, const TwkTemporalRectify* rp, const float* colour, const float* moments, const float* geometry,
                              const float* historyColour, const float* historyMoments, const float* historyGeometry, const TwkCameraDefinition* historyCamera,
                              const float* previousPositions, int width, int height, float* colourOut, float* momentsOut, float* trustOut);
int twk_temporal_cascade_carried_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                                      const float* historyGeometry, const TwkCameraDefinition* historyCamera, const float* trust, const float* previousPositions,
                                      int width, int height, float* layersOut);
/* EXPLICIT form of twk_temporal_accumulate (rp NULL; trustOut must then be NULL) or of twk_temporal_accumulate_rectified (rp given),
 * with a table: motion is a DEVICE pointer to numMotion records, 16-byte aligned, indexed by instance; an instance beyond the table
 * is unmoved. motion NULL or numMotion 0 launches the existing kernels: byte for byte the existing call. Otherwise, per candidate
 * pixel, g' = X g for a moved instance (no history unless g' is finite), the projection and the taps' position test run on g', and
 * everything after is the existing merge. All refusals of those calls apply; also TWK_ERROR_INVALID_VALUE: current NULL (there is
 * no own-buffer form: the own-buffer calls build their table themselves), numMotion < 0, a table that is not 16-byte aligned, an
 * output that overlaps the table. Asynchronous on the handle's stream; the table is read by the launch, not copied. */
int twk_temporal_accumulate_moving(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalRectify* rp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                                   const TwkInstanceMotion* motion, int numMotion, int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut);
/* twk_temporal_accumulate_cascade (trust NULL) or twk_temporal_accumulate_cascade_trusted (trust given) with a table, as above. */
int twk_temporal_accumulate_cascade_moving(TwkDevice dev, const TwkTemporal* tp, const TwkCascade* cp, const void* currentLayers, const void* currentGeometry,
                                           const void* historyLayers, const void* historyGeometry, const TwkCameraDefinition* historyCamera, const void* trust,
                                           const TwkInstanceMotion* motion, int numMotion, int width, int height, void* layersOut);
/* Pure CPU, no device: the same definitions compiled for the host, on host arrays as twk_temporal_rectify_host and
 * twk_temporal_cascade_trusted_host take them; motion is a HOST array of numMotion records (NULL or 0: none, and the results are
 * those of the existing host forms). rp NULL: the plain merge (trustOut must be NULL); trust NULL: the untrusted cascade merge. */
int twk_temporal_moving_host(const TwkTemporal* tp, const TwkTemporalRectify* rp, const float* colour, const float* moments, const float* geometry,
                             const float* historyColour, const float* historyMoments, const float* historyGeometry, const TwkCameraDefinition* historyCamera,
                             const TwkInstanceMotion* motion, int numMotion, int width, int height, float* colourOut, float* momentsOut, float* trustOut);
int twk_temporal_cascade_moving_host(const TwkTemporal* tp, const TwkCascade* cp, const float* currentLayers, const float* currentGeometry, const float* historyLayers,
                                     const float* historyGeometry, const TwkCameraDefinition* historyCamera, const float* trust, const TwkInstanceMotion* motion, int numMotion,
                                     int width, int height, float* layersOut);
/* OWN-BUFFER and ASSEMBLED forms (twk_temporal_accumulate, twk_temporal_accumulate_rectified, twk_temporal_accumulate_assembled,
 * twk_temporal_accumulate_assembled_rectified): while every instance's transform is bit-equal to the one it had when the history
 * was taken — the only state there is without twk_update_instance_transform — they launch what they always launched. Otherwise
 * they build the table on the host (twk_instance_motion per instance), upload it to a buffer of the handle (freed with the
 * history) and launch the Moving builds, the cascade's own-buffer merge included. This call hands out the table the last such
 * merge used: *count records, 0 if it used none; host may be NULL when capacity is 0. TWK_ERROR_INVALID_VALUE: a NULL handle or
 * count, a capacity below the count (*count is written all the same: a first call with capacity 0 asks for it). On tiles, twk_assemble_devices_with_geometry refuses (TWK_ERROR_INVALID_STATE) a source handle
 * whose instance transforms are not bit-equal to the primary's. */
int twk_read_temporal_motion(TwkDevice dev, TwkInstanceMotion* host, size_t capacity, int* count);

/* ---- Assembling a tiled frame — new calls, ABI stays 9, no existing struct changes; without them no kernel and no bit of any
 * picture changes ----------------------------------------------------------------------------------------------------------------
 * With distribution 1 and several devices every handle renders its checkerboard share into packed launchWidth x H buffers: the
 * beauty, the two AOVs, the moments, the sample counts and the cascade's layers. twk_assemble moves every requested plane and layer
 * of every source device into full W x H buffers on ONE handle (`primary`) in ONE kernel launch, so that what works on whole
 * pictures (the twk_denoise* calls with explicit buffers, twk_cascade_resolve with explicit layers, twk_estimate_noise with explicit
 * moments) has something to work on. The map is twk_tile_column's; the complete definition is csrc/assemble_device.h and
 * tests/assemble_restate.py restates it in numpy. Padding columns (x >= width) are neither read nor written. What it is NOT: a
 * scatter back to the tiles (adaptive selection and planning stay per device), a seventh plane for the geometry AOV (the
 * _with_geometry forms below assemble it), or a path for the shared-frame strategies (their beauty is already whole, their other planes are not).
 *   plane                     element                                   assembled buffer
 *   TWK_PLANE_OUTPUT          the output format's pixel, 16 or 8 B       [H][W]
 *   TWK_PLANE_ALBEDO/NORMAL   the output format's pixel, 16 or 8 B       [H][W]
 *   TWK_PLANE_MOMENTS         float4, always                             [H][W]
 *   TWK_PLANE_SAMPLE_COUNTS   uint32                                     [H][W]
 *   TWK_PLANE_CASCADE         float4, K layers [K][H][launchWidth]       [K][H][W]  (the shape twk_cascade_resolve's explicit form takes) */
enum { TWK_PLANE_OUTPUT = 0, TWK_PLANE_ALBEDO = 1, TWK_PLANE_NORMAL = 2, TWK_PLANE_MOMENTS = 3, TWK_PLANE_SAMPLE_COUNTS = 4, TWK_PLANE_CASCADE = 5, TWK_PLANE_COUNT = 6 };
#define TWK_PLANE_BIT(plane) (1u << (plane))
/* One source device's packed buffers, indexed by TWK_PLANE_*; the planes that are not requested are not looked at. */
typedef struct TwkAssemblySource { const void* plane[TWK_PLANE_COUNT]; } TwkAssemblySource;
/* planeMask: TWK_PLANE_BIT(p) ored together. sources[d] holds the buffers of the device with index d of deviceCount, which must be
 * primary's device count; every pointer must be addressable from primary's device (the form an RCCL caller uses: pointers into the
 * block it gathered). Asynchronous on primary's stream. The assembled buffers belong to primary, are allocated at first use and
 * sized by its state, output format and cascade layer count; a later call overwrites them. One device is legal: the identity map
 * cropped to width.
 * TWK_ERROR_INVALID_VALUE: a NULL handle (before any HIP call), an empty or unknown plane mask, NULL sources, a NULL source pointer
 * of a requested plane, a deviceCount that is not primary's. TWK_ERROR_INVALID_STATE: before twk_set_state, distribution 0 with
 * several devices (every handle holds the whole frame), a requested plane whose switch is off on primary (twk_enable_aov,
 * twk_enable_moments, twk_enable_adaptive, twk_enable_cascade). */
int twk_assemble(TwkDevice primary, unsigned int planeMask, const TwkAssemblySource* sources, int deviceCount);
/* The in-process form: the handles' own buffers, devices[] in any order. Recorded launches of every handle are rendered first.
 * Ordered without a host synchronisation: an event recorded on every source stream is waited for on primary's stream, and the
 * sources' streams wait for the assembly before they render on. Peers are read directly where hipDeviceCanAccessPeer allows (peer
 * access is enabled, "already enabled" is fine), else staged with hipMemcpyPeerAsync into a block on primary; TWK_ASSEMBLE_STAGE=1
 * in the environment when primary is created forces the staging path.
 * Beyond twk_assemble's refusals. TWK_ERROR_INVALID_VALUE: a NULL entry, handles that disagree with primary in resolution, tile
 * size, distribution, device count, output format or cascade parameters, indices that are not each of 0..count-1 exactly once.
 * TWK_ERROR_INVALID_STATE: a handle before twk_set_state, a requested plane whose switch is off on some handle, TWK_PLANE_OUTPUT
 * from a handle that renders into a shared frame (twk_set_shared_frame). */
int twk_assemble_devices(TwkDevice primary, unsigned int planeMask, const TwkDevice* devices, int count);
/* The assembled buffer of one plane on primary and its size in bytes; valid until the next change of shape. twk_read_assembled
 * copies it to the host as it is (bytes must be its size) and synchronises. TWK_ERROR_INVALID_STATE: the plane has not been assembled
 * since the handle was created or since twk_set_state changed resolution, tile size or distribution, twk_set_output_format changed
 * the format, or twk_enable_cascade changed the layers: those drop every assembled buffer. */
int twk_get_assembled_device_pointer(TwkDevice primary, int plane, void** dptr, size_t* bytes);
int twk_read_assembled(TwkDevice primary, int plane, void* host, size_t bytes);
/* The same two forms with the geometry AOV of every tile share (twk_render_geometry_tile) in the same ONE launch: further entries of
 * the same table (16-byte elements, one layer), the same event ordering, peer access and staging. The geometry is no seventh plane
 * (TWK_PLANE_COUNT stays 6, bit 6 stays unknown): it has an assembled W x H float4 buffer of its own on primary,
 * twk_get_assembled_geometry_device_pointer / twk_read_assembled_geometry (numFloats = width*height*4; synchronises). That buffer
 * is freed whenever the other assembled buffers are, and is marked stale — the two getters and twk_temporal_accumulate_assembled
 * refuse it — by whatever invalidates primary's own geometry AOV: a change of its camera 0, state or scene. planeMask may be 0 here:
 * the geometry alone; otherwise it means what it means above.
 * twk_assemble_with_geometry: geometrySources[d] is device d's packed launchWidth x H geometry, addressable from primary's device.
 * twk_assemble_devices_with_geometry: the handles' own geometry buffers.
 * Beyond the refusals above. TWK_ERROR_INVALID_STATE: the geometry off on primary (both forms) or on some handle; in the handle
 * form, a handle whose geometry is not valid (no twk_render_geometry_tile since its camera, state or scene changed).
 * TWK_ERROR_INVALID_VALUE: NULL geometrySources or a NULL entry of it; in the handle form, a handle whose camera 0 is not
 * primary's, byte for byte. The explicit form cannot see the sources' cameras or age: that is the caller's to keep.
 * There is no twk_assemble_geometry_host: twk_assemble_host with elementBytes 16 and layers 1 is that. */
int twk_assemble_with_geometry(TwkDevice primary, unsigned int planeMask, const TwkAssemblySource* sources, const void* const* geometrySources, int deviceCount);
int twk_assemble_devices_with_geometry(TwkDevice primary, unsigned int planeMask, const TwkDevice* devices, int count);
int twk_get_assembled_geometry_device_pointer(TwkDevice primary, void** dptr, size_t* bytes);
int twk_read_assembled_geometry(TwkDevice primary, float* host, size_t numFloats);
/* Host only, no handle: the same definition over host arrays. sources[d] is device d's [layers][height][launchWidth] elements of
 * elementBytes (4, 8 or 16) with launchWidth as twk_set_state derives it: width for one device, else twk_launch_width(width,
 * tileSize[0], deviceCount); destination is [layers][height][width] elements, of which exactly the in-picture ones are written.
 * TWK_ERROR_INVALID_VALUE: a NULL argument or source, a count or size below 1, a tile size that is no power of two, another
 * elementBytes. */
int twk_assemble_host(const void* const* sources, int deviceCount, int width, int height, const int tileSize[2], int elementBytes, int layers, void* destination);

/* ---- measurement -------------------------------------------------------------------------- */
int twk_profile_enable(TwkDevice dev, int enable);   /* hipEvent pair around every kernel launch */
int twk_profile_reset(TwkDevice dev);
int twk_profile_get(TwkDevice dev, float msPerKernelClass[TWK_KERNEL_COUNT], int launchesPerKernelClass[TWK_KERNEL_COUNT]);
int twk_stats_enable(TwkDevice dev, int enable);     /* counting kernel variants (not for timed runs) */
int twk_stats_get(TwkDevice dev, TwkLaunchStats* stats, int reset);
int twk_stream_peak_gbps(TwkDevice dev, size_t bytes, int repeats, float* gbps); /* float4 copy kernel */
/* Divergent-gather ceiling: every lane of every wave chases its own chain of 128-byte lines through a table of
 * tableBytes and reads each line as eight 16-byte loads (the access pattern of a wide-node fetch); returns giga
 * lane-loads (16 B each) per second. With a table the size of the scene this is the memory-side ceiling of traversal. */
int twk_gather_peak(TwkDevice dev, size_t tableBytes, float* gigaLaneLoadsPerSecond);

/* ---- debugging / parity taps (stage-level SoA read-back after one launch) ------------------ */
/* First-bounce hit record per pixel of the last launch: t, beta, gamma, instance, primitive.
 * Requires twk_debug_capture(dev, 1) before the launch. prim/inst = -1 on miss. */
int twk_debug_capture(TwkDevice dev, int enable);
int twk_debug_read_first_hits(TwkDevice dev, float* tBetaGamma /*3 per px*/, int* instPrim /*2 per px*/, size_t numPixels);

/* The raw samples of the last wavefront pass as its accumulate kernel read them: [samples of the pass][launchWidth*height] float4
 * (radiance rgb, w = 0 for a launch index outside the image), sample s of the pass being iteration (first iteration of the pass)
 * + s. Deferred launches are rendered first; synchronises. TWK_ERROR_INVALID_STATE before any pass, and after a call that
 * overwrote the path streams (twk_debug_trace_queue, a reallocation). The tests of the luminance moments fold these. */
int twk_debug_read_path_radiance(TwkDevice dev, float* host, size_t numFloats);

/* Which builds of the shade kernel ran. The dispatcher picks one of 128 launcher slots per shade launch from seven flags: bit 0
 * ENV (spherical environment), 1 TEX (some material has an albedo texture), 2 PRIMARY (first launch of a pass that computes its
 * own primary rays), 3 LDS_TABLES (instance + material + light tables fit the block's LDS budget), 4 MEASURE (statistics or time
 * view), 5 SORT (class-ordered windows), 6 SLIM (TWK_STREAMS_SLIM). twk_debug_shade_builds: the slots launched on this handle
 * since the last reset, bit I of mask[I / 64]; deferred launches are enqueued first. Recorded on the host, one OR per launch.
 * twk_debug_shade_build_slots: the slots that hold a build at all (no handle, no GPU needed); a test that wants every build
 * launched reads the set from here. New calls only, ABI stays 9. */
int twk_debug_shade_builds(TwkDevice dev, uint64_t mask[2], int reset);
int twk_debug_shade_build_slots(uint64_t mask[2]);

/* Closest-hit / any-hit query of arbitrary rays through the device BVH (≙ optixTrace contract,
 * raygeneration.cu:84-89, closesthit.cu:281-286). rays: 8 floats each (o.xyz, tmin, d.xyz, tmax).
 * out: t, beta, gamma per ray; ids: instance, primitive (or -1). anyHit != 0: ids[0] = 1 if occluded.
 * Geometric query: cutout opacity is not applied here. */
int twk_trace_rays(TwkDevice dev, const float* rays, size_t numRays, int anyHit, float* tBetaGamma, int* ids);

/* The same query through the PERSISTENT traversal kernel of the hot path, as ONE bounce's launch sees it: closestRays go
 * into the radiance ray queue, shadowRays into the shadow queue (either may be empty; 8 floats per ray as above).
 * tBetaGammaSlot: t, beta, gamma and the bits of the hit triangle's slot per closest ray (the hit record shade reads;
 * twk_debug_read_acceleration maps a slot to its primitive); instance: -1 on a miss; occluded: 1 / 0 per shadow ray.
 * Overwrites the handle's path streams; not for scenes with cutout opacity. */
int twk_debug_trace_queue(TwkDevice dev, const float* closestRays, size_t numClosest, const float* shadowRays, size_t numShadow,
                          float* tBetaGammaSlot, int* instance, int* occluded);

/* Read-back of the acceleration structure twk_build produced, for the same-BVH host walker of the test tooling
 * (oracle/same_bvh_walk.cpp: visit counts and a one-core traversal rate on exactly the tree the kernels walk).
 * Two-call protocol: with NULL buffers only `info` is filled. wideNodes: numNodes x 64 B, the quantised 4-ary nodes the
 * persistent kernel walks (four float4: origin.xyz, cell.x | cell.y, cell.z, qlo.x, qlo.y | qlo.z, qhi.x, qhi.y, qhi.z |
 * four references; q words hold one byte per child, child box = origin + q * cell, an unused entry has the inverted box
 * lo 255 / hi 0; reference >= 0 inner node, < 0 leaf with payload ~ref = instance index, or first slot | (count - 1) << 28
 * [| 0x40000000 for world-space slots]);
 * triangles: numTriangleSlots x 48 B (three float4: vertex, .w = primitive index / instance index / 0);
 * instances: numInstances x 128 B (world-to-object 3x4, BVH root, ..., see csrc/device_types.h DevInstance). */
typedef struct TwkAccelerationInfo
{
  int      root;      /* node index traversal starts at */
  int      twoLevel;  /* 0: every instance is flattened, no instance reference occurs */
  uint64_t numNodes, numTriangleSlots, numInstances;
  int      root2;     /* ABI 7: the second wide node of an 8-wide root (a ray starts at `root` with `root2` on its stack), -1: none */
  int      nodeFloats; /* ABI 8: floats per node record: 16 = quantised 4-ary node (64 B), 20 = compressed 8-ary node (80 B, root = node 0, csrc/device_types.h) */
} TwkAccelerationInfo;
int twk_debug_read_acceleration(TwkDevice dev, TwkAccelerationInfo* info, void* wideNodes, void* triangles, void* instances);

/* Host copy of everything the kernels read of the scene, for the host build of the kernels (oracle/host_kernels.cpp: the
 * north_star's "single-threaded C++ CPU fallback of the same kernels", test infrastructure like the oracle): writes the
 * handle's launch parameters (csrc/device_types.h LaunchParams, `paramsBytes` must equal its size) with every SCENE pointer
 * (binary nodes, triangle slots, shading records, instances, materials, lights, camera, textures, environment tables)
 * replaced by a pointer into host memory owned by the handle (valid until the next twk_build / twk_debug_snapshot_scene /
 * twk_device_destroy); the path streams, counters and output pointers are null. Nothing in the product reads it back. */
int twk_debug_snapshot_scene(TwkDevice dev, void* launchParams, size_t paramsBytes);

/* Unit taps of the device math used by the shaders (bit-exact parity with the oracle):
 * op 0 sin, 1 cos, 2 exp, 3 atan2(x[i], y[i]), 4 acos, 5 atan, 6 sqrt, 7 1/x, 8 log, 9 pow(x[i], y[i]). */
int twk_debug_math(TwkDevice dev, int op, const float* x, const float* y, float* out, size_t n);

/* The traversal kernel's short divisions (csrc/trace_device.h exactReciprocal, exactQuotients: v_rcp_f32 and fused corrections in
 * place of the 11-instruction IEEE expansion) against the compiler's own `/`, both computed in one kernel.
 * mode 0: the reciprocal of the `count` bit patterns first, first + 1, ... (count <= 2^32; x, d unused);
 * mode 1: the quotients x[i] / d[i] and the reciprocal 1 / d[i] of `count` caller's pairs, |x[i]| <= |d[i]| as woopSetup has them;
 * mode 2: the same over `count` pairs drawn on the device from the seed `first` (half with |d| in [0.5, 1), half over every binade;
 *         x up to 70 binades below d, denormals and zeros included).
 * mismatches: results that differ from `/` in any bit (two NaNs count as equal); fallbacks: operands outside the proven range,
 * which the helpers hand to `/` themselves; offenders: the first eight mismatching operands, two words each (mode 0: the bit
 * pattern, 0; otherwise the bits of x and of d), may be NULL. Serves the tests; no rendering path calls it. New call only, ABI stays 9. */
int twk_debug_exact_division(TwkDevice dev, int mode, uint32_t first, uint64_t count, const float* x, const float* d,
                             uint64_t* mismatches, uint64_t* fallbacks, uint32_t offenders[16]);

/* ---- host scene layer (rtigo3 Application: description files, meshes, camera) -------------- */
typedef struct TwkApp_t* TwkApp;

/* ≙ Application::loadSystemDescription (Application.cpp:1046-1299) + createCameras/createLights
 * (:562-677) + loadSceneDescription (:1397-1878). */
int twk_app_create(TwkApp* out, const char* systemDescriptionFile, const char* sceneDescriptionFile);
int twk_app_create_from_strings(TwkApp* out, const char* systemDescription, const char* sceneDescription);
int twk_app_destroy(TwkApp app);

typedef struct TwkAppInfo
{
  int   strategy, devicesMask, light, miss, lensShader, samplesSqrt;
  int   resolution[2], tileSize[2], pathLengths[2];
  float epsilonFactor, envRotation, clockFactor;
  float center[3], phi, theta, fov, distance;
  int   numCameras, numLights, numMaterials, numGeometries, numInstances;
  int   shaderVariant; /* "shaderVariant" of the system description (grammar extension): TWK_SHADERS_*; applied by twk_app_init_device */
  int   nextEventEstimation; /* ABI 9: "nextEventEstimation 0|1" (grammar extension ≙ USE_NEXT_EVENT_ESTIMATION), default 1; applied by twk_app_init_device */
  int   debugExceptions;     /* ABI 9: "debugExceptions 0|1" (grammar extension ≙ USE_DEBUG_EXCEPTIONS), default 0 */
} TwkAppInfo;

int twk_app_info(TwkApp app, TwkAppInfo* info);
/* "outputFormat 0|1" of the system description (grammar extension ≙ Optix7Gui USE_FP32_OUTPUT: 1 = TWK_OUTPUT_HALF4),
 * default 0; applied by twk_app_init_device. */
int twk_app_get_output_format(TwkApp app, int* format);
/* "denoiser 0|1|2|3" (0 = off, default; else inputKind + 1), "denoiserIterations n", "denoiserSigmas color normal albedo" of
 * the system description (grammar extensions ≙ Optix7Gui's denoiser switches, app_config.h): *enabled and the parameters
 * twk_denoise is to be called with (twk_denoiser_defaults where a key is absent; demodulateAlbedo 0 for TWK_DENOISER_RGB).
 * twk_app_init_device enables the AOVs when the key asks for a guided kind. */
int twk_app_get_denoiser(TwkApp app, int* enabled, TwkDenoiser* dn);
/* "denoiserVariance 0|1" (default 0), "denoiserFirefly k", "denoiserSigmaLuminance sigma": *enabled = the description asks for
 * twk_denoise_variance in place of twk_denoise (it takes effect when "denoiser" is on), and its parameters
 * (twk_denoiser_variance_defaults where a key is absent). */
int twk_app_get_denoiser_variance(TwkApp app, int* enabled, TwkDenoiserVariance* dv);
/* "denoiserSampledVariance 0|1" (default 0), "denoiserMinSamples n" (n >= 2; default TWK_DENOISER_MIN_SAMPLES): *enabled = the
 * description asks for twk_denoise_variance_sampled with *minSamples (it takes effect when "denoiser" is on, with the parameters of
 * twk_app_get_denoiser_variance, whatever "denoiserVariance" says). twk_app_init_device enables the moments when the key asks. */
#define TWK_DENOISER_MIN_SAMPLES 4
int twk_app_get_denoiser_sampled(TwkApp app, int* enabled, int* minSamples);
/* "denoiserGeometry 0|1" (default 0), "denoiserSigmaPosition s", "denoiserInstanceStop 0|1": *enabled = the description asks for
 * twk_denoise_geometry in the mode the other keys choose (it takes effect where "denoiser 3" is on), and its parameters
 * (twk_denoiser_geometry_defaults where a key is absent). twk_app_init_device enables the geometry AOV when the key asks. */
int twk_app_get_denoiser_geometry(TwkApp app, int* enabled, TwkDenoiserGeometry* dg);
/* The stopping rule: "targetNoise e" (default 0 = off; e > 0 and finite), "targetNoiseQuantile q" (default 0.95; in (0, 1]),
 * "targetNoiseInterval n" (default 16; n >= 1). A value outside its range drops the line with a warning. *enabled = a target is
 * set: a render loop then calls twk_estimate_noise on every device after every *interval iterations, merges the summaries and ends
 * at the first check where valid > 0 and twk_noise_quantile(*quantile) <= *target (rtigo3_hip -m 1 does; INTEGRATION.md "The
 * stopping rule"). twk_app_init_device enables the moments when a target is set. */
int twk_app_get_target_noise(TwkApp app, int* enabled, float* target, float* quantile, int* interval);
/* "adaptiveSampling 0|1" (default 0) and "adaptiveMaxSamples n" (default 4096; n >= 1; a value outside drops the line with a
 * warning). *enabled = the description asks for adaptive sampling AND sets a target ("adaptiveSampling 1" without "targetNoise" is
 * dropped with a warning); *ap: target, minSamples and darkFloor as the stopping rule uses them, maxSamples from the description.
 * twk_app_init_device enables moments and adaptive sampling when the key is on (rtigo3_hip -m 1 runs the loop; INTEGRATION.md "The
 * adaptive loop"). */
int twk_app_get_adaptive(TwkApp app, int* enabled, TwkAdaptive* ap);
/* "adaptiveBudget 0|1" (default 0), "adaptiveMinBatch n" and "adaptiveMaxBatch n" (defaults: twk_adaptive_plan_defaults; a value that
 * breaks 1 <= adaptiveMinBatch <= adaptiveMaxBatch <= 64 drops the line with a warning). *enabled = the key is on AND adaptive
 * sampling itself is enabled (twk_app_get_adaptive); rtigo3_hip -m 1 then runs the planned loop (INTEGRATION.md "The adaptive loop"). */
int twk_app_get_adaptive_plan(TwkApp app, int* enabled, TwkAdaptivePlan* plan);
/* "fireflyCascade 0|1" (default 0), "fireflyCascadeLayers n", "fireflyCascadeStart s", "fireflyCascadeBase b", "fireflyCascadeKappa k"
 * (defaults: twk_cascade_defaults, twk_cascade_resolve_defaults; a value twk_enable_cascade or twk_cascade_resolve would refuse
 * drops the line with a warning, thresholds that reach inf drop layers, start and base together). The keys are written back only
 * when they differ from off / the defaults. twk_app_init_device enables the cascade when the key is on; the render loop resolves
 * (INTEGRATION.md "The firefly cascade"). */
int twk_app_get_cascade(TwkApp app, int* enabled, TwkCascade* cp, TwkCascadeResolve* rp);
/* "tileAssembly 0|1" (default 0; any other value draws a warning and leaves it off), written back only when on. On, with several
 * devices and strategy 3, rtigo3_hip -m 1 assembles the planes its post steps need with one twk_assemble_devices and runs them on
 * the assembled frame (INTEGRATION.md "Assembling a tiled frame"); with strategy 1 or 2 it refuses the run. */
int twk_app_get_tile_assembly(TwkApp app, int* enabled);
/* The moving-camera loop of rtigo3_hip -m 1: "temporalAccumulation 0|1" (default 0), "temporalFrames n" (1..4096, default 1),
 * "temporalOrbitStep f" (the fraction of a full turn added to the camera's phi per frame; finite; default
 * TWK_TEMPORAL_ORBIT_STEP, provisional), "temporalMaxHistory n" (>= 1) and "temporalPositionTolerance t" (>= 0, finite; defaults:
 * twk_temporal_defaults). A value outside its range drops the line with a warning; the keys are written back only when they differ
 * from off / the defaults. With the key on, frame f = 0..frames-1 renders samplesSqrt^2 iterations from the camera at phi + f x
 * step under the sample offset f x samplesSqrt^2, renders the geometry and merges (on several devices: tile shares, one assembly
 * with geometry, the assembled merge); INTEGRATION.md "The temporal seam on several devices". twk_app_init_device enables moments
 * and geometry when the key is on. */
#define TWK_TEMPORAL_ORBIT_STEP 0.001f
int twk_app_get_temporal(TwkApp app, int* enabled, TwkTemporal* tp, int* frames, float* orbitStep);
/* The rectified merge in that loop: "temporalRectify 0|1" (default 0: the loop merges with twk_temporal_accumulate; 1: with
 * twk_temporal_accumulate_rectified, on several devices twk_temporal_accumulate_assembled_rectified), "temporalRectifyGamma g"
 * (>= 0, finite), "temporalRectifyRadius r" (1..4), "temporalRectifyMinTaps n" (>= 2; defaults: twk_temporal_rectify_defaults). A
 * value outside its range drops the line with a warning; the keys are written back only when they differ from the defaults.
 * keys: how many of the four keys the description holds — rtigo3_hip refuses any of them without "temporalAccumulation 1", before
 * a device is created. */
int twk_app_get_temporal_rectify(TwkApp app, int* enabled, TwkTemporalRectify* rp, int* keys);
/* An object that moves in that loop: "temporalInstanceStep <idInstance> <dx> <dy> <dz>" (idInstance >= 0, a finite step; another line
 * is dropped with a warning). Before every frame after the first, rtigo3_hip translates that instance by one more step with
 * twk_update_instance_transform on every device; the merges then carry its history along ("Moving an object" above). *idInstance
 * -1: the description has no such key. rtigo3_hip refuses the key without "temporalAccumulation 1", for an id beyond the scene's
 * instances and for an instance that carries a light. TwkAppInfo is unchanged. */
int twk_app_get_temporal_motion(TwkApp app, int* idInstance, float step[3]);
/* "selectiveUpdate 0|1" of the system description (default 0; written back only when on): a render loop sets
 * twk_set_update_mode(dev, TWK_UPDATE_SELECTIVE) on every device before twk_app_init_device, so that the updates of
 * "temporalInstanceStep" are selective ("Selective instance updates" above). TWK_ERROR_INVALID_VALUE: a NULL argument. */
int twk_app_get_selective_update(TwkApp app, int* enabled);
int twk_app_set_resolution(TwkApp app, int width, int height); /* re-derives the camera frustum (aspect) */
int twk_app_get_state(TwkApp app, TwkDeviceState* state);
int twk_app_get_cameras(TwkApp app, TwkCameraDefinition* out, int capacity);
int twk_app_get_lights(TwkApp app, TwkLightDefinition* out, int capacity);
int twk_app_get_materials(TwkApp app, TwkMaterialGUI* out, int capacity);
int twk_app_get_geometry_sizes(TwkApp app, int idGeometry, size_t* numAttributes, size_t* numIndices);
int twk_app_get_geometry(TwkApp app, int idGeometry, TwkTriangleAttributes* attributes, unsigned int* indices);
/* Flattened instance list in traverseNode order (Device.cpp:1283-1331). */
int twk_app_get_instance(TwkApp app, int idInstance, int* idGeometry, float transform[12], int* idMaterial, int* idLight);
/* Runs the reference's init sequence on a device: setState, initCameras, initLights, initMaterials,
 * initScene (Application.cpp:303,328-332). */
int twk_app_init_device(TwkApp app, TwkDevice dev);
/* ≙ the text Application::saveSystemDescription writes (Application.cpp:1300-1345): the current settings in the
 * loader's grammar. Two-call protocol: out == NULL returns the length (without the terminator) in *length. */
int twk_app_system_description(TwkApp app, char* out, size_t capacity, size_t* length);
/* Tonemapper settings of the system description ("gamma", "colorBalance", "whitePoint", "burnHighlights",
 * "crushBlacks", "saturation", "brightness", Application.cpp:1244-1292). */
int twk_app_get_tonemapper(TwkApp app, TwkTonemapper* tm);
/* ≙ the file name Application::screenshot builds (Application.cpp:2235-2239, getDateTime :1927-2010):
 * <prefixScreenshot>_<spp>spp_<YYYMMDD_HHMMSS_mmm>.png|.hdr (tm_year and tm_mon as the reference prints them). */
int twk_app_screenshot_path(TwkApp app, int tonemap, char* out, size_t capacity);

/* Image files written by Application::screenshot through DevIL (Application.cpp:2251-2320), without DevIL:
 * 8-bit RGB PNG (stored deflate blocks) and Radiance RGBE .hdr (flat scanlines). `bottomUp` != 0: row 0 of the
 * buffer is the BOTTOM row of the picture (the renderer's convention, IL_ORIGIN_LOWER_LEFT). */
/* ≙ Picture::load + the format expansion of Texture::create* (Picture.cpp:231-560, Texture.cpp:933-1042): decode an
 * image file to RGBA32F, row 0 = bottom row, ready for twk_init_texture. PNG, baseline JPEG (libjpeg's default
 * decode path, byte-exact), Radiance .hdr, PFM — DevIL is not available. Two-call protocol: with rgba == NULL only width/height are returned; otherwise
 * capacityFloats must be >= width*height*4. */
int twk_load_image(const char* path, int* width, int* height, float* rgba, size_t capacityFloats);
/* File name given with "envMap" in the system description (Application.cpp:1151-1156), "" if none. */
int twk_app_get_environment(TwkApp app, char* out, size_t capacity);
int twk_write_png_rgb8(const char* path, int width, int height, const unsigned char* rgb8, int bottomUp);
int twk_write_hdr_rgba32f(const char* path, int width, int height, const float* rgba, int bottomUp);

/* Stand-alone host helpers (≙ sg::Triangles::create*, Camera::getFrustum, calculateTileShift). */
int twk_mesh_plane(unsigned int tessU, unsigned int tessV, unsigned int upAxis, TwkTriangleAttributes* attr, size_t* numAttr, unsigned int* idx, size_t* numIdx);
int twk_mesh_box(TwkTriangleAttributes* attr, size_t* numAttr, unsigned int* idx, size_t* numIdx);
int twk_mesh_sphere(unsigned int tessU, unsigned int tessV, float radius, float maxTheta, TwkTriangleAttributes* attr, size_t* numAttr, unsigned int* idx, size_t* numIdx);
int twk_mesh_torus(unsigned int tessU, unsigned int tessV, float innerRadius, float outerRadius, TwkTriangleAttributes* attr, size_t* numAttr, unsigned int* idx, size_t* numIdx);
int twk_mesh_parallelogram(const float position[3], const float vecU[3], const float vecV[3], const float normal[3], TwkTriangleAttributes* attr, size_t* numAttr, unsigned int* idx, size_t* numIdx);
int twk_camera_frustum(const float center[3], float phi, float theta, float fov, float distance, float aspect, TwkCameraDefinition* out); /* ≙ Camera::getFrustum Camera.cpp:187-216 */
/* Tile map ≙ distribute() raygeneration.cu:152-164: launch column → pixel column. */
int twk_tile_column(int launchX, int launchY, const int tileSize[2], int deviceCount, int deviceIndex, int* pixelX);
int twk_launch_width(int width, int tileSizeX, int deviceCount, int* launchWidth); /* ≙ DeviceMultiGPULocalCopy.cpp:84-97 */
/* Tokenise description text like Parser::getNextToken (Parser.cpp:72-148): writes "<type> <token>\n" per token
 * (type 1 = identifier, 2 = value) into out (NUL terminated), returns the count in numTokens. */
int twk_parse_tokens(const char* text, char* out, size_t capacity, int* numTokens);

#ifdef __cplusplus
}
#endif

#endif /* TWEEKER_HIP_H */

// The handle behind the C ABI (TwkDevice_t) and what the host files that implement the ABI share: device_api.hip (handle, setters,
// readers), device_scene.hip (scene and build), device_pass.hip (streams and the wavefront pass in its three forms: uniform, listed, planned — shade_device.h "the samples of a thread"), device_post.hip (compositor,
// tonemap, denoiser, noise estimate), device_temporal.hip (the temporal merge, plain and rectified), device_adaptive.hip (adaptive sampling: switch, select, readers), device_cascade.hip (the firefly cascade: switch, layers, resolve), device_temporal_cascade.hip (the cascade's layers through the temporal merge), device_assemble.hip (assembling a tiled frame, with or without its geometry AOV), device_debug.hip (measurement and parity taps). Internal: no kernel file includes it.
// Device memory has one home. Every buffer the handle allocates is a DeviceArray member (device_buffers.h: pointer + capacity in
// elements, freed by its destructor), so a new buffer is one member and one ensure() where it is used, and twk_device_destroy
// lists none. A result picture kept for readers is a DevicePicture (ensurePicture, currentPicture). "The handle's own X, or
// nothing" is ownOutput / ownAlbedo / ownNormal / ownMoments / ownGeometry / ownSampleCounts. Every reader ends in readBack (or
// its tail copyBack), every twk_get_*_device_pointer is getPointer. Borrowed pointers (d_outputExternal) and the pinned, mapped
// h_dropped / d_dropped stay plain fields.
#pragma once
#include "device_types.h"
#include "bvh_build.h"
#include "denoise_device.h"
#include "temporal_device.h"
#include "noise_device.h"
#include "adaptive_device.h"
#include "adaptive_plan_device.h"
#include "cascade_device.h"
#include "temporal_cascade_device.h"
#include "temporal_rectify_device.h"
#include "assemble_device.h"
#include "device_buffers.h"
#include "update_plan.h"
#include "light_motion.h"

#include <memory>
#include <string>
#include <vector>

namespace twk {
void launchTrace(const LaunchParams& p, int depth, bool count, const TraceBuild& build, int gridBlocks, hipStream_t stream);
void launchTraceQuery(const LaunchParams& p, const float* rays, unsigned int numRays, int anyHit, float* tBetaGamma, int* ids, int gridBlocks, hipStream_t stream);
int launchShade(const LaunchParams& p, int depth, bool primary, int gridBlocks, hipStream_t stream);
void shadeBuildSlots(uint64_t mask[2]);
void launchTileEntries(const LaunchParams& p, const float4* topTable, int tilesX, int tilesY, int4* out, hipStream_t stream);
// generateKernel / accumulateKernel for a pass of the form `samples`: UniformSamples, ListedSamples or PlannedSamples (shade_device.h
// "the samples of a thread"; shade_kernels.hip instantiates the three). half: RGBA16F buffers; cascade.layers != nullptr: the cascade is on.
template<typename Samples> void launchGenerate(const LaunchParams& p, const Samples& samples, hipStream_t stream);
template<typename Samples> void launchAccumulate(const LaunchParams& p, bool half, const Samples& samples, const CascadeOn& cascade, hipStream_t stream);
void launchCompositor(const void* tiles, void* output, bool half, int width, int height, int launchWidth, int deviceCount,
                      int tileSizeX, int tileShiftX, int tileShiftY, hipStream_t stream);
void launchMathTap(int op, const float* x, const float* y, float* out, size_t n, hipStream_t stream);
void launchExactDivisionTap(int mode, unsigned int first, unsigned long long count, const float* x, const float* d, unsigned long long* tally /* 18 words, zeroed */, hipStream_t stream);
void launchStreamCopy(const float4* src, float4* dst, size_t n, hipStream_t stream);
void launchGatherProbeFill(float4* table, size_t count, unsigned int lines, hipStream_t stream);
void launchGatherProbe(const float4* table, unsigned int lines, int steps, float* out, int gridBlocks, hipStream_t stream);
void launchTonemap(const void* hdr, bool half, unsigned char* ldr, size_t numPixels, const TwkTonemapper& tm, hipStream_t stream);
void launchDenoisePrepare(const void* beauty, const void* albedo, const void* normal, bool half, float4* colour, float4* guideNormal, float4* guideAlbedo,
                          const DenoiseConstants& k, hipStream_t stream);
void launchDenoiseMoments(int kind, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k, const float4* sampled, float minSamples, hipStream_t stream,
                          const float4* geometry = nullptr, const DenoiseGeometryConstants* g = nullptr);
void launchDenoiseLevel(int kind, bool lds, bool variance, const float4* in, const float4* guideNormal, const float4* guideAlbedo, float4* out, const DenoiseConstants& k, int step, hipStream_t stream,
                        const float4* geometry = nullptr, const DenoiseGeometryConstants* g = nullptr);
void launchDenoiseFinish(const void* beauty, bool half, const float4* colour, const float4* guideNormal, const float4* guideAlbedo, void* denoised, const DenoiseConstants& k, hipStream_t stream);
void launchGeometry(const LaunchParams& p, float4* geometry, bool tiled, int gridBlocks, hipStream_t stream);
// temporal_carry_kernels.hip
void launchGeometryMotion(const LaunchParams& p, float4* geometry, float4* plane, const TwkInstanceMotion* motion, unsigned int numMotion, const TwkInstanceCarry* carry,
                          unsigned int numCarry, const float4* previousPositions, int gridBlocks, hipStream_t stream);
void launchTemporal(const void* colour, bool half, const float4* moments, const float4* geometry, const float4* historyColour, const float4* historyMoments,
                    const float4* historyGeometry, void* colourOut, float4* historyOut, float4* momentsOut, const TemporalConstants& k, hipStream_t stream,
                    const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u, const float4* carried = nullptr);
unsigned int* launchAdaptiveSelect(const float4* moments, const unsigned int* counts, size_t numElements, unsigned int* active, void* scratch,
                                   const AdaptiveConstants& k, int numCUs, hipStream_t stream);
unsigned long long* launchAdaptivePlan(const float4* moments, const unsigned int* counts, size_t numElements, unsigned int* active, unsigned int* pathOffset,
                                       void* scratch, const AdaptiveConstants& k, const AdaptivePlanConstants& plan, int numCUs, hipStream_t stream);
void launchNoise(const float4* moments, size_t numElements, float* errorMap, TwkNoiseSummary* summary, const NoiseConstants& k, int numCUs, hipStream_t stream);
void launchCascadeResolve(const CascadeConstants& k, float kappa, const float4* layers, float* lambda, int width, int height, void* resolved, bool half, hipStream_t stream);
void launchTemporalCascade(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, float4* layersOut,
                           const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream, const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u, const float4* carried = nullptr);
void launchTemporalCascadeTrusted(const float4* layers, const float4* geometry, const float4* historyLayers, const float4* historyGeometry, const float* trust, float4* layersOut,
                                  const TemporalConstants& k, const CascadeConstants& c, hipStream_t stream, const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u, const float4* carried = nullptr);
void launchTemporalRectify(const void* colour, bool half, const float4* moments, const float4* geometry, const float4* historyColour, const float4* historyMoments,
                           const float4* historyGeometry, float4* scratchA, float4* scratchB, void* colourOut, float4* historyOut, float4* momentsOut, float* trustOut,
                           const TemporalConstants& k, const RectifyConstants& r, hipStream_t stream, const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u, const float4* carried = nullptr);
void launchAssemble(const AssembleShape& s, const AssembleTable& table, int count, hipStream_t stream);
}

using namespace twk;

static_assert(sizeof(TwkCameraDefinition) == 48, "CameraDefinition is 48 B (camera_definition.h:34-40)");
static_assert(sizeof(TwkLightDefinition) == 80, "LightDefinition is 80 B (light_definition.h:42-59)");
static_assert(sizeof(TwkTriangleAttributes) == 48, "TriangleAttributes is 48 B (vertex_attributes.h:34-40)");
static_assert(sizeof(DevLight) == sizeof(TwkLightDefinition), "device light layout");
static_assert(sizeof(DevMaterial) == 64, "MaterialDefinition is 64 B (material_definition.h:37-56)");
static_assert(sizeof(DevInstance) == 128, "instance record");
static_assert(sizeof(BvhNode) == 64, "BVH2 node");

// What a geometry holds on the device beside its slice of d_attributes once a device-pointer source has written that slice
// (vertex_source_device.h; device_vertex_source.hip). mirrorStale: the slice is newer than GeometryHost::attributes — every reader of
// the mirror calls refreshMirror first, and an upload of the mirror is skipped (the slice is what it would bring). The adjacency table
// of the frames is built at the first call that recomputes them; d_kept holds the previous positions while
// TwkDevice_t::previousOnDevice says so. All of it goes with the geometry (twk_clear_scene).
struct GeometryDevice
{
  bool mirrorStale = false;
  DeviceArray<unsigned int> d_adjacencyOffsets, d_adjacencyTriangles;
  DeviceArray<float4> d_kept;
};

struct GeometryHost
{
  std::vector<TwkTriangleAttributes> attributes; // the host mirror of the geometry's slice of d_attributes (stale: GeometryDevice)
  std::unique_ptr<GeometryDevice> device;
  std::vector<unsigned int>          indices;
  unsigned int attributeBase = 0, indexBase = 0;
  int triangleBase = 0, nodeBase = 0, numTriangles = 0;
  float rootBounds[6];
};

struct InstanceHost
{
  int   geometry;
  float transform[12];
  int   material, light;
};

struct TimedLaunch { hipEvent_t start, stop; int kind; };
// What a table of primary-ray entry points (trace_kernels.hip tileEntryKernel) was built for: camera bits, frame, tree, tile
// distribution. Compared with memcmp (as floats, TWK_NODE_CACHED | 1 rounded to TWK_NODE_CACHED | 0, a build serial
// stopped counting at 2^24, and -0.0 compared equal to +0.0).
struct TileEntriesKey
{
  uint32_t camera[12];
  int32_t  resolution[2], topRoot, topRoot2, launchWidth, deviceCount, deviceIndex, tileSize[2], valid;
  uint64_t buildSerial;
};
#define TWK_STATS_WORDS 192 // device words of TwkLaunchStats: [0, 24) traversal + shade totals, [24, 96) the shade phases (shade_device.h PhaseScope); twice: the time view's scratch copy
#define TWK_COUNTER_WORDS (TWK_COUNTERS_PER_DEPTH * (TWK_MAX_DEPTH + 2)) // one lane's counter block

// A result picture the handle keeps for its readers: width x height pixels in the output format it was made in, `valid` once a
// call has written it (ensurePicture and currentPicture, below the handle)
struct DevicePicture
{
  DeviceArray<void> pixels; int width = 0, height = 0, format = TWK_OUTPUT_FLOAT4; bool valid = false;
  size_t count() const { return (size_t) width * height; }
  bool shaped(int w, int h, int f) const { return pixels != nullptr && width == w && height == h && format == f; }
  void release() { pixels.release(); width = height = 0; valid = false; }
};

struct TwkDevice_t
{
  int ordinal = 0, index = 0, count = 1, miss = 1;
  int numCUs = 256;
  hipStream_t stream = nullptr;

  TwkDeviceState state;
  bool stateSet = false;
  int  launchWidth = 1;

  std::vector<TwkCameraDefinition> cameras;
  std::vector<TwkLightDefinition>  lights;
  std::vector<DevMaterial>         materials;
  std::vector<GeometryHost>        geometries;
  std::vector<InstanceHost>        instances;
  bool built = false;
  bool twoLevel = true;                 // some instance is entered through the top level (else the soup is the whole scene)
  int  flattenMaxTriangles = TWK_FLATTEN_TRIANGLES, flattenMaxReferences = TWK_FLATTEN_REFERENCES;
  int  maxInstanceMaterial = -1, maxInstanceLight = -1; // largest indices the built scene's instances use
  TwkBuildInfo buildInfo;

  // device memory
  DeviceArray<float> d_camera;
  DeviceArray<DevLight> d_lights;
  DeviceArray<DevMaterial> d_materials;
  DeviceArray<float> d_attributes; DeviceArray<unsigned int> d_indices;
  DeviceArray<BvhNode> d_nodes, d_wideNodes /* build-time only: full-precision wide nodes, freed once quantised */; DeviceArray<float4> d_wideQ, d_triangles, d_shadeTriangles; DeviceArray<DevInstance> d_instances;
  bool directSmallLeaves = true; /* TWK_DIRECT_SMALL_LEAVES=0: A/B */ bool costedCuts = true; /* TWK_COSTED_CUTS=0: A/B */ bool fusedPrimary = true; /* TWK_FUSED_PRIMARY=0: A/B */ bool tileEntries = true; /* TWK_TILE_ENTRIES=0: A/B */ bool wideRoot = true; /* TWK_WIDE_ROOT=0: A/B */ int wideRoot1 = 0, wideRoot2 = TWK_BVH_SENTINEL; size_t wideNodesTotal = 0;
  DeviceArray<int4> d_tileEntries; TileEntriesKey tileEntriesKey = {}; uint64_t buildSerial = 0; // entry points of the primary rays (trace_kernels.hip tileEntryKernel) and what they were built for
  DeviceArray<float4> d_topNodes, d_topNodes7; bool topCache = true; int traceWavesForced = 0 /* TWK_TRACE_WAVES_RUNTIME: 6 or 7, 0 = by scene */; // TWK_TOP_CACHE=0 turns the LDS top-of-tree cache off (A/B)
  DeviceArray<float4> d_texels[3];
  DeviceArray<float> d_envCDF_U, d_envCDF_V;
  int tlasRoot = 0;
  size_t totalNodes = 0, totalTriangles = 0;

  // per-resolution streams
  DeviceArray<void> d_streamBlock; // one allocation carved into the SoA streams; its capacity: the paths of the largest pass it holds
  // output and AOV running means: RGBA32F, or RGBA16F in the same (float4-typed) pointers when outputFormat is TWK_OUTPUT_HALF4
  int outputFormat = TWK_OUTPUT_FLOAT4; // twk_set_output_format (≙ Optix7Gui USE_FP32_OUTPUT, app_config.h:57-59)
  DeviceArray<float4> d_outputInternal; // its capacity in pixels is what the other per-launch-index buffers grow to
  float4* d_outputExternal = nullptr; size_t outputExternalBytes = 0;
  bool outputFrame = false; // the external buffer is a shared full frame (twk_set_shared_frame)
  DeviceArray<unsigned int> d_counters;
  DeviceArray<unsigned long long> d_stats;
  unsigned int* h_dropped = nullptr; unsigned int* d_dropped = nullptr; // pinned + device-mapped: LaunchParams::droppedPushes
  DeviceArray<int> d_spill;
  bool packedQueue = true; // TWK_PACKED_QUEUE=0: A/B
  bool slimStreams = true; // TWK_SLIM_STREAMS=0: A/B (device_types.h LaunchParams::slimSlotBits)
  bool trianglePairs = true; DeviceArray<float4> d_trianglePairs; // TWK_TRIANGLE_PAIRS=0: A/B (device_types.h "triangle pairs"); the records, empty when no reference names one
  uint64_t shadeBuilds[2] = {0, 0}; // the shadeKernel builds launched since the last reset, by launcher index (twk_debug_shade_builds)
  int shadeSort = 1;      // TWK_SHADE_SORT=0: slot order (A/B); 1: class order in every launch but the first of a pass; 2: in the first too
  DeviceArray<float4> d_firstHit; DeviceArray<int> d_firstHitInstance;
  // denoiser AOVs (Optix7Gui raygeneration.cu:125-164): per-path values of a pass and their running means per launch index
  bool aovEnabled = false; int shaderVariant = TWK_SHADERS_RTIGO3;
  bool nextEventEstimation = true, debugExceptions = false; // twk_set_next_event_estimation / twk_set_debug_exceptions (≙ shaders/config.h:50-56)
  bool timeView = false; DeviceArray<float> d_pathTime; // twk_set_time_view
  DeviceArray<float4> d_pathAlbedo, d_pathNormal;
  DeviceArray<float4> d_aovAlbedo, d_aovNormal;
  // twk_enable_moments: luminance moments (mean, M2, n, 0) of the samples per launch index, always f32 (LaunchParams::moments)
  bool momentsEnabled = false; DeviceArray<float4> d_moments;
  unsigned int sampleOffset = 0; // twk_set_sample_offset (LaunchParams::sampleOffset)
  // twk_enable_cascade: the firefly cascade's layers, [cascade.layers][launchWidth x height] float4, exactly that many (the layer
  // stride), always f32; the resolve's lambda stream (floats, shared by both forms) and the internal resolved picture of the
  // own-buffer form
  bool cascadeEnabled = false; TwkCascade cascadeParameters = {TWK_CASCADE_LAYERS, TWK_CASCADE_START, TWK_CASCADE_BASE}; CascadeConstants cascadeK = {};
  DeviceArray<float4> d_cascade;
  DeviceArray<float> d_cascadeLambda;
  DevicePicture resolved;
  // twk_enable_geometry: the geometry AOV (world position, instance + 1) per launch index, always f32; geometryValid: rendered by
  // twk_render_geometry since the last change of camera, state or scene
  bool geometryEnabled = false; DeviceArray<float4> d_geometry; bool geometryValid = false;
  // twk_temporal_accumulate, own-buffer form: two sets of three f32 streams (colour, moments, geometry) — the set temporalKept holds
  // what the last call kept (its camera: temporalCamera), the other receives this call's — and the merged colour, the picture
  // whose shape the streams share
  DeviceArray<float4> d_temporal[2][3]; DevicePicture temporalColour;
  int temporalKept = 0; bool temporalHasHistory = false;
  TwkCameraDefinition temporalCamera;
  // twk_update_instance_transform keeps the history, so beside its camera the history has the transform of every instance as of
  // its frame (temporalTransforms, 12 floats each, refreshed when a merge swaps the history). A merge that finds an instance
  // elsewhere builds the table of temporal_motion_device.h on the host (temporalMotion; empty: the last own-buffer merge used
  // none — twk_read_temporal_motion) and uploads it to d_temporalMotion, grown while idle. All dropped by dropTemporal.
  std::vector<float> temporalTransforms;
  std::vector<TwkInstanceMotion> temporalMotion; DeviceArray<TwkInstanceMotion> d_temporalMotion;
  // twk_update_geometry_vertices keeps the history too: the first update of a geometry since the history's frame keeps its positions
  // as of that frame (previousPositions[geometry], one float4 per vertex; empty: not deformed), until a merge swaps the history or
  // dropTemporal drops it. twk_render_geometry_motion (temporal_carry_device.h) uploads them packed (d_previousPositions) with the two
  // records per instance and writes the previous-position plane beside the geometry AOV; previousPlaneValid goes with geometryValid.
  // previousOnDevice[geometry]: the vector has its size (what says "deformed", and what the bases are summed from) but its content
  // lives in the geometry's d_kept, written by the ingest kernel of a device-pointer source; twk_render_geometry_motion packs it with
  // a device-to-device copy. Cleared with previousPositions.
  std::vector<std::vector<float4>> previousPositions; std::vector<char> previousOnDevice;
  DeviceArray<float4> d_previousPositions, d_previousPlane; DeviceArray<TwkInstanceMotion> d_carryMotion; DeviceArray<TwkInstanceCarry> d_carry;
  bool previousPlaneValid = false;
  // what d_carryMotion and d_carry hold, and whether d_previousPositions holds previousPositions as they are: the uploads and the wait
  // after them are skipped while nothing has changed since the last plane
  std::vector<TwkInstanceMotion> carryMotionUploaded; std::vector<TwkInstanceCarry> carryUploaded; bool previousPositionsUploaded = false;
  // twk_temporal_accumulate_rectified (temporal_rectify_device.h): the two scratch streams its first launch writes and its second
  // reads, shared by the explicit and the own-buffer form; and the own-buffer form's trust plane, one
  // float per pixel of the temporal result, valid while the last own-buffer merge was a rectified one. Freed by dropTemporal.
  DeviceArray<float4> d_rectify[2];
  DeviceArray<float> d_temporalTrust; bool temporalTrustValid = false;
  // twk_temporal_enable_cascade: while temporalCascade is set the own-buffer twk_temporal_accumulate also merges the handle's cascade
  // layers (temporal_cascade_device.h) with the same previous geometry and camera, into two sets of [temporalCascadeLayers]
  // [pixels of the frame] float4 — the set temporalCascadeKept holds what the last call kept, the other receives this call's.
  // Dropped with the temporal history (dropTemporal) and by twk_enable_cascade off or with new parameters.
  bool temporalCascade = false; DeviceArray<float4> d_temporalCascade[2];
  int temporalCascadeLayers = 0, temporalCascadeKept = 0; bool temporalCascadeHasHistory = false, temporalCascadeValid = false;
  int lastPassCount = 0, lastPassPixels = 0; // samples per launch index and launch indices of the last pass, while its pathRadiance stream still holds them (twk_debug_read_path_radiance); 0: none
  // twk_denoise: the internal denoised picture (≙ m_d_denoisedBuffer, Optix7Gui Application.cpp:2478) and the four f32 streams
  // of the filter (colour ping, colour pong, normal guide, albedo guide; denoise_device.h) in one array
  DevicePicture denoised;
  DeviceArray<float4> d_denoiseStreams;
  // twk_estimate_noise: the summary the kernel adds into (noise_device.h), zeroed on the stream before each launch; noiseValid: an estimate has been issued
  DeviceArray<TwkNoiseSummary> d_noise; bool noiseValid = false;
  // twk_enable_adaptive: per launch index the iteration its next adaptive sample uses (d_sampleCounts) and the ascending list of
  // the launch indices the last twk_adaptive_select chose (d_active, numActive of them), both launchWidth x height words, and the
  // select's scan scratch (adaptive_device.h adaptiveScratchBytes of as many elements as its capacity says; also the explicit form's).
  //   uniformNext     the index after the last iteration a flushed twk_launch rendered
  //   countsCurrent   d_sampleCounts says what the picture holds; else it is filled with uniformNext before it is read
  //   adaptiveStarted an adaptive pass has run since the last restart: the picture is no longer uniform, twk_launch(i != 0) is refused
  //   activeValid     d_active is the list of a select that nothing has invalidated since
  bool adaptiveEnabled = false; DeviceArray<unsigned int> d_sampleCounts, d_active;
  DeviceArray<void> d_adaptiveScratch;
  unsigned int uniformNext = 0, numActive = 0; bool countsCurrent = false, adaptiveStarted = false, activeValid = false;
  // twk_adaptive_plan, own-buffer form: the plan's list and path offsets (adaptive_plan_device.h) in buffers of their own, n
  // and n + 1 words, so that a plan leaves the select's list what it is. The plan's scratch is d_adaptiveScratch, grown to
  // adaptivePlanScratchBytes of its elements (never less than the select's): adaptiveScratchPlan. planValid: d_planActive / d_planOffsets are the plan of a call that
  // nothing has invalidated since — what drops a list drops it, a select does, and the planned pass that renders it does (the
  // counts advance in the pass, so a plan is rendered once).
  DeviceArray<unsigned int> d_planActive, d_planOffsets;
  bool adaptiveScratchPlan = false;
  unsigned int planActive = 0, planPaths = 0; bool planValid = false;
  // twk_assemble / twk_assemble_devices with this handle as primary: the assembled W x H buffer of every plane (d_assembled[plane],
  // of exactly the bytes of the output format / the cascade layers it was allocated for; assembledValid: assembled since it was allocated), the
  // staging block of the peers that cannot be read directly, and the two events that order the streams without a host
  // synchronisation: assembleReady is recorded on this handle's stream as a source, assembleDone on it as primary.
  DeviceArray<void> d_assembled[TWK_PLANE_COUNT];
  bool assembledValid[TWK_PLANE_COUNT] = {false, false, false, false, false, false};
  DeviceArray<void> d_assembleStage; bool assembleStage = false; // TWK_ASSEMBLE_STAGE=1: every source is staged (tests both paths on one GPU)
  hipEvent_t assembleReady = nullptr, assembleDone = nullptr;
  // twk_assemble_with_geometry / twk_assemble_devices_with_geometry: the assembled W x H geometry AOV, float4. It is no seventh
  // plane (TWK_PLANE_COUNT stays 6): freed with the other assembled buffers (dropAssembled), and stale (assembledGeometryValid
  // false, the buffer kept) once this handle's camera, state or scene changes — staleGeometry, which is what clears geometryValid
  DeviceArray<void> d_assembledGeometry; bool assembledGeometryValid = false;
  int denoiseGeometryLdsMaxStep = 16; // the same border for the GEO builds (twk_denoise_geometry, four streams per tap): staged also wins at steps 8 and 16, by 0.04 ms each at 1080p (profiles/r20_denoise_geometry.md); steps above 16 are not measured and stay direct; TWK_DENOISE_LDS_MAX_STEP sets both
  int denoiseLdsMaxStep = 4; // levels of a step up to this run the LDS-staged build, larger steps the direct-load build (measured per step: DESIGN.md 4.3); TWK_DENOISE_LDS_MAX_STEP (A/B): 0 = every level direct, 128 = every level staged
  bool captureFirstHits = false;
  bool statsEnabled = false;
  bool profileEnabled = false;
  std::vector<TimedLaunch> timed; size_t timedUsed = 0;
  float profileMs[TWK_KERNEL_COUNT] = {0, 0, 0, 0, 0};
  int   profileLaunches[TWK_KERNEL_COUNT] = {0, 0, 0, 0, 0};
  // Deferred launches: twk_launch only records the iteration; consecutive iterations are rendered together as one
  // wavefront pass of up to batchMax samples per pixel when the batch is full or anything observes the device.
  int   batchMax = 64;
  size_t streamBudgetBytes = 0; // TWK_STREAM_BUDGET_MB: cap on the path streams of one pass (0 = device memory is the limit)
  unsigned int pendingFirst = 0;
  int   pendingCount = 0;

  // Pass lanes: a wavefront pass may be cut into up to TWK_MAX_LANES independent sub-passes over disjoint path ranges, each a
  // chain of generate / trace / shade launches on a stream of its own (lane 0 = `stream`), joined before the accumulate
  // kernel. Small passes are bound by the dependent-launch chain and the longest ray of each launch, not by throughput:
  // two chains side by side fill each other's gaps (renderPass).
  hipStream_t laneStream[TWK_MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t  laneDone[TWK_MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t  laneFork = nullptr;
  int   lanesForced = 0; // TWK_PASS_LANES: 0 = choose by pass size
  int   laneTraceWaves = 0; // TWK_LANE_TRACE_WAVES: trace blocks per CU of each lane (0 = TWK_TRACE_WAVES / lanes)

  // Selective instance updates (include/tweeker_hip.h; device_scene.hip updateSelective). updateMode: twk_set_update_mode, read by
  // the next build. kept.valid: the built scene was built in selective mode and its by-products are still here — d_wideNodes (above),
  // d_nodeCost (with costedCuts) and d_pairFlags (with pairs) on the device, and on the host the layout, per tree its box, payload,
  // height and SAH terms, and the build primitives of every geometry. A full-mode build holds none of it past its end (KeptScope).
  // KeptBuild is also the working state of a build: buildScene fills a local one through the stage functions updateSelective amends
  // this one with, and moves it here, valid, when a selective-mode build has succeeded.
  // d_updateSoup / d_updateRanges / d_updateResult: scratch of the updates, grown on demand.
  // sahBuilt / refits (twk_refit_geometry_vertices, TwkRefitInfo): sahInner + sahLeaf as of the tree's last real build, and the refits
  // it has taken since; every real build of the tree writes fresh terms and so resets both
  struct TreeTerms { double sahInner = 0.0, sahLeaf = 0.0; int height = 0; double sahBuilt = 0.0; int refits = 0; };
  struct KeptBuild
  {
    bool valid = false, pairs = false, pairRewrite = false;
    SceneLayout layout;
    std::vector<TreeTerms> geometryTerms, instanceTerms; // per entered geometry's tree, per flattened instance's tree
    std::vector<float4> boxLo, boxHi; std::vector<int> leafPayload; int topHeight = 0;
    std::vector<std::vector<int>> primFirst;
    void clear() { *this = KeptBuild(); }
  } kept;
  int updateMode = TWK_UPDATE_FULL;
  DeviceArray<float> d_nodeCost; DeviceArray<int> d_pairFlags;
  DeviceArray<int4> d_updateSoup; DeviceArray<int2> d_updateRanges; DeviceArray<int> d_updateResult;
  TwkUpdateInfo updateInfo = {}; bool updateInfoValid = false;
  // the twk_refit_* calls: what the last refit did (valid until the next build), and the scratch of a call's batch (bvh_build.h refitSceneScratchWords)
  TwkRefitInfo refitInfo = {}; bool refitInfoValid = false;
  DeviceArray<unsigned int> d_refitScratch;
  DeviceArray<unsigned int> d_sourceCheck; // one word: the lowest vertex of a device-pointer source whose position is not finite
  // twk_enable_emitter_motion (light_motion.h): while emitterMotion is set the transform calls accept an instance that carries a
  // light and move its definition with it, always from the light's anchor (lightAnchors[light], grown on demand; dropLightAnchors)
  bool emitterMotion = false;
  std::vector<LightAnchor> lightAnchors;

  std::vector<std::vector<char>> hostScene; // twk_debug_snapshot_scene: host copies of the scene arrays

  LaunchParams params;
  BvhBuilder builder;
};

// The camera, the state or the scene changed: the handle's geometry AOV and the geometry it assembled as a primary are of the old one
inline void staleGeometry(TwkDevice dev) { dev->geometryValid = false; dev->assembledGeometryValid = false; dev->previousPlaneValid = false; }

// Every light's anchor goes (twk_init_lights, twk_build, twk_clear_scene): the next move of an emitter anchors anew
inline void dropLightAnchors(TwkDevice dev) { dev->lightAnchors.clear(); }

// Whether the handle holds previous positions of some geometry (twk_update_geometry_vertices since the history's frame)
inline bool geometryDeformed(TwkDevice dev)
{
  for (const std::vector<float4>& kept : dev->previousPositions) if (!kept.empty()) return true;
  return false;
}

// Bytes of one output / AOV pixel in the handle's output format: RGBA32F 16, RGBA16F 8 (Optix7Gui Half4)
inline size_t pixelBytes(int format) { return (format == TWK_OUTPUT_HALF4) ? 8 : sizeof(float4); }
inline size_t pixelBytes(TwkDevice dev) { return pixelBytes(dev->outputFormat); }
inline bool halfOutput(TwkDevice dev) { return dev->outputFormat == TWK_OUTPUT_HALF4; }
// Pixels of the buffer the handle accumulates into: the shared W x H frame, or its packed launchWidth x H buffer
inline size_t outputPixels(TwkDevice dev)
{
  return (size_t) ((dev->d_outputExternal && dev->outputFrame) ? dev->state.resolution[0] : dev->launchWidth) * dev->state.resolution[1];
}

// The handle's launch indices: the elements of each of its per-launch-index buffers
inline size_t launchIndices(TwkDevice dev) { return (size_t) dev->launchWidth * dev->state.resolution[1]; }

// "The handle's own X, or nothing": the stream when its switch is on and it holds at least n elements, else nullptr. What else a
// caller asks of it (geometryValid, "a packed tile buffer is no picture") is the caller's check, with its own text.
template<typename T> inline T* ownStream(bool enabled, const DeviceArray<T>& stream, size_t n) { return (enabled && stream.holds(n)) ? stream.get() : nullptr; }
inline float4* ownAlbedo(TwkDevice dev, size_t n) { return ownStream(dev->aovEnabled, dev->d_aovAlbedo, n); }
inline float4* ownNormal(TwkDevice dev, size_t n) { return ownStream(dev->aovEnabled, dev->d_aovNormal, n); }
inline float4* ownMoments(TwkDevice dev, size_t n) { return ownStream(dev->momentsEnabled, dev->d_moments, n); }
inline float4* ownGeometry(TwkDevice dev, size_t n) { return ownStream(dev->geometryEnabled, dev->d_geometry, n); }
inline unsigned int* ownSampleCounts(TwkDevice dev, size_t n) { return ownStream(dev->adaptiveEnabled, dev->d_sampleCounts, n); }
// ... and the buffer the handle accumulates into, the caller's or its own, once the internal one holds n pixels (it has no switch)
inline float4* ownOutput(TwkDevice dev, size_t n = 0)
{
  if (dev->d_outputInternal.capacity() < n) return nullptr;
  return dev->d_outputExternal ? dev->d_outputExternal : dev->d_outputInternal.get();
}

// Grows a scratch array that launches on the handle's stream may still use: everything enqueued runs before it is freed
template<typename T> inline int growIdle(TwkDevice dev, DeviceArray<T>& array, size_t count, size_t bytes = 0)
{
  if (array.holds(count)) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  return array.allocate(count, false, nullptr, bytes);
}

// `picture` as width x height pixels of the handle's output format. One of another shape or format (compared exactly, not "large
// enough"), or none, is freed once everything enqueued has run and allocated again, not valid.
inline int ensurePicture(TwkDevice dev, DevicePicture& picture, int width, int height)
{
  if (picture.shaped(width, height, dev->outputFormat)) return TWK_SUCCESS;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  picture.release();
  const int rc = picture.pixels.allocate((size_t) width * height * pixelBytes(dev)); if (rc) return rc;
  picture.width = width; picture.height = height; picture.format = dev->outputFormat;
  return TWK_SUCCESS;
}
// The picture for a reader: nullptr unless a call has written it and it is in the current output format
inline void* currentPicture(TwkDevice dev, const DevicePicture& picture)
{
  return (picture.valid && picture.format == dev->outputFormat) ? picture.pixels.get() : nullptr;
}

// Whether the byte ranges [a, a + aBytes) and [b, b + bBytes) share a byte; a NULL pointer overlaps nothing
inline bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes)
{
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t) a, y = (uintptr_t) b;
  return x < y + bBytes && y < x + aBytes;
}
inline bool overlaps(const void* a, const void* b, size_t bytes) { return overlaps(a, bytes, b, bytes); }

// What a reader copies to the host: `count` elements of `elementBytes` at `source`; source nullptr: there is nothing to read and
// the call is refused with `refusal`. elementBytes 0: pixels of the output format, widened exactly to RGBA32F (readPixels).
// ownShape: the count is the source's own (a result's width x height), so that without a source there is no size to hold the
// caller's against and the refusal comes first; else the count is the state's, and the caller's size is checked first.
struct Readback { const void* source; const char* refusal; size_t count, elementBytes; bool ownShape; };

// Helpers more than one of the files needs; each is defined in the file that owns it
namespace twk {
// device_pass.hip
int activate(TwkDevice dev, const char* where, bool flush = true);
int calculateShift(int size);
TraceBuild traceBuild(TwkDevice dev, bool primary);
void refreshParams(TwkDevice dev);
int slimSlotBits(TwkDevice dev);
int ensureStreams(TwkDevice dev, int samples = 1);
int checkDroppedPushes(TwkDevice dev, const char* where);
void dropAdaptive(TwkDevice dev);
int currentSampleCounts(TwkDevice dev);
int ensureStreamsForPaths(TwkDevice dev, size_t paths);
// device_api.hip
int setSwitch(TwkDevice dev, const char* where, bool TwkDevice_t::*flag, int enable);
int readPixels(TwkDevice dev, const void* src, void* host, size_t numPixels, bool raw);
int copyBack(TwkDevice dev, const char* name, const void* source, size_t count, size_t elementBytes, void* host, bool dropped = false);
int readBack(TwkDevice dev, const char* name, const Readback& r, void* host, size_t given, size_t unit, const char* sizeText, bool dropped = false);
// device_temporal.hip
void dropTemporal(TwkDevice dev);
// device_temporal_carry.hip
void keepPreviousPositions(TwkDevice dev, int idGeometry);
void dropPreviousPositions(TwkDevice dev, bool release);
// device_vertex_source.hip
int refreshMirror(TwkDevice dev, int idGeometry);
int ingestVertexSource(TwkDevice dev, const char* name, bool refit, int idGeometry, const TwkVertexSource* source, size_t numVertices);
// its two halves, for twk_refit_scene, which checks every entry before it writes any: what the check and ingest launches are given
struct VertexSourceView { const void* pointer = nullptr; size_t stride = 0; bool records = false, recompute = false; };
int checkVertexSource(TwkDevice dev, const std::string& where, int idGeometry, const TwkVertexSource* source, size_t numVertices, VertexSourceView& view);
int storeVertexSource(TwkDevice dev, int idGeometry, const VertexSourceView& view);
inline bool mirrorStale(const GeometryHost& g) { return g.device && g.device->mirrorStale; }
// device_temporal.hip
int temporalParameters(const char* name, const TwkTemporal* tp, TemporalConstants& k);
int temporalHistoryCamera(const char* name, const TwkCameraDefinition& camera, TemporalConstants& k);
// device_cascade.hip
CascadeOn cascadeFold(TwkDevice dev);
// device_temporal_cascade.hip
void dropTemporalCascade(TwkDevice dev);
const char* temporalCascadeRefusal(TwkDevice dev);
int temporalCascadeOwn(TwkDevice dev, const TemporalConstants& k, const float4* layers, const float4* geometry, const float4* historyGeometry, const float* trust = nullptr,
                       const TwkInstanceMotion* motion = nullptr, unsigned int numMotion = 0u, const float4* carried = nullptr);
// device_assemble.hip
void dropAssembled(TwkDevice dev);
}

// One twk_get_*_device_pointer: source(pointer, size) is the entry point's own check and answer, run on the active handle once
// the argument is known to be there; what it returns but TWK_SUCCESS is the call's refusal
template<typename Source> inline int getPointer(TwkDevice dev, const char* name, void** dptr, size_t* bytes, const Source& source)
{
  int rc = activate(dev, name); if (rc) return rc;
  if (!dptr) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": NULL argument");
  void* pointer = nullptr; size_t size = 0;
  if ((rc = source(pointer, size))) return rc;
  *dptr = pointer;
  if (bytes) *bytes = size;
  return TWK_SUCCESS;
}

// Host scene layer: what rtigo3's Application builds before it hands the scene to the per-GPU Device.
//   system description  ≙ Application::loadSystemDescription   reference src/Application.cpp:1046-1299
//   lights + light mesh ≙ Application::createLights            reference src/Application.cpp:572-677
//   scene description   ≙ Application::loadSceneDescription    reference src/Application.cpp:1397-1878
//   instance flattening ≙ Device::traverseNode/multiplyMatrix  reference src/Device.cpp:1265-1331
// No GUI, no image loading, no assimp (out of scope); "model assimp" lines are skipped
// with a warning.
#pragma once
#include "../../../include/tweeker_hip.h"
#include "orbit_camera.h"
#include "triangle_meshes.h"

#include <map>
#include <memory>
#include <string>
#include <vector>

namespace twk {

// Minimal scene graph with the reference's node kinds (inc/SceneGraph.h:47-133).
struct SceneNode
{
  enum Kind { GROUP, INSTANCE, TRIANGLES } kind;
  explicit SceneNode(Kind k) : kind(k) {}
  virtual ~SceneNode() {}
};

struct TrianglesNode : SceneNode
{
  explicit TrianglesNode(unsigned int id_) : SceneNode(TRIANGLES), id(id_) {}
  unsigned int id;
  TriangleMesh mesh;
};

struct InstanceNode : SceneNode
{
  InstanceNode() : SceneNode(INSTANCE)
  {
    for (int i = 0; i < 12; ++i) transform[i] = 0.0f;
    transform[0] = transform[5] = transform[10] = 1.0f;
  }
  int   material = -1;
  int   light    = -1;
  float transform[12];
  std::shared_ptr<SceneNode> child;
};

struct GroupNode : SceneNode
{
  GroupNode() : SceneNode(GROUP) {}
  std::vector<std::shared_ptr<InstanceNode>> children;
};

struct FlatInstance
{
  int   geometry;
  float transform[12];
  int   material;
  int   light;
};

class Application
{
public:
  Application();

  bool loadSystemDescription(const std::string& text, std::string& error);
  bool loadSceneDescription(const std::string& text, std::string& error);
  // Runs createCameras/createLights, parses the scene and flattens it. Call once after the system description.
  bool buildScene(const std::string& sceneText, std::string& error);

  void setResolution(int w, int h);
  std::string systemDescription() const;
  TwkDeviceState deviceState() const;

  // system options (Application.cpp:55-75,105-120 defaults)
  int   strategy      = 0;
  int   devicesMask   = 255;
  int   interop       = 0;
  bool  present       = false;
  int   light         = 0;
  int   miss          = 1;
  int   lensShader    = 0;
  int   nextEventEstimation = 1; // grammar extension "nextEventEstimation": ≙ USE_NEXT_EVENT_ESTIMATION (shaders/config.h:50-52)
  int   debugExceptions = 0;     // grammar extension "debugExceptions": ≙ USE_DEBUG_EXCEPTIONS (config.h:54-56)
  int   outputFormat = 0;        // grammar extension "outputFormat": TWK_OUTPUT_*, 1 ≙ Optix7Gui USE_FP32_OUTPUT 0 (app_config.h:57-59)
  // grammar extensions "denoiser" (0 off, else TwkDenoiser::inputKind + 1), "denoiserIterations", "denoiserSigmas" (colour, normal,
  // albedo): where Optix7Gui's display path calls optixDenoiserInvoke (Application.cpp:942-1001); the values are
  // twk_denoiser_defaults' until a key sets them
  int   denoiser = 0;
  int   denoiserIterations = 3;
  float denoiserSigmas[3] = {8.0f, 0.3f, 0.1f};
  // "denoiserVariance" (1: twk_denoise_variance in place of twk_denoise), "denoiserFirefly", "denoiserSigmaLuminance": the
  // variance-guided, firefly-clamping mode; twk_denoiser_variance_defaults' values until a key sets them
  int   denoiserVariance = 0;
  float denoiserFirefly = 3.0f;
  float denoiserSigmaLuminance = 4.0f;
  // "denoiserSampledVariance" (1: twk_denoise_variance_sampled, the measured variance of the samples where a pixel has seen at
  // least "denoiserMinSamples" of them), TWK_DENOISER_MIN_SAMPLES until a key sets it
  int   denoiserSampledVariance = 0;
  int   denoiserMinSamples = TWK_DENOISER_MIN_SAMPLES;
  // "denoiserGeometry" (1: twk_denoise_geometry, the geometry guide, where "denoiser 3" is on), "denoiserSigmaPosition",
  // "denoiserInstanceStop": twk_denoiser_geometry_defaults until a key sets them
  int   denoiserGeometry = 0;
  float denoiserSigmaPosition = TWK_DENOISER_SIGMA_POSITION;
  int   denoiserInstanceStop = 0;
  // "targetNoise" (0: off; else the render loop ends once the "targetNoiseQuantile" quantile of twk_estimate_noise's relative
  // standard error is at most this), checked every "targetNoiseInterval" iterations
  float targetNoise = 0.0f;
  float targetNoiseQuantile = 0.95f;
  int   targetNoiseInterval = 16;
  // "adaptiveSampling" (1: between the stopping rule's checks the render loop samples only the pixels twk_adaptive_select picks
  // by "targetNoise"; dropped without a target), "adaptiveMaxSamples" (no pixel is selected once it has this many samples)
  // "fireflyCascade" (1: the accumulate kernels fold the firefly cascade's layers, twk_enable_cascade, and a render loop resolves
  // them, twk_cascade_resolve, before it shows or denoises the picture), "fireflyCascadeLayers", "fireflyCascadeStart",
  // "fireflyCascadeBase" (TwkCascade), "fireflyCascadeKappa" (TwkCascadeResolve)
  int   fireflyCascade = 0;
  int   fireflyCascadeLayers = TWK_CASCADE_LAYERS;
  float fireflyCascadeStart = TWK_CASCADE_START, fireflyCascadeBase = TWK_CASCADE_BASE, fireflyCascadeKappa = TWK_CASCADE_KAPPA;
  // "tileAssembly" (1: a several-device render loop assembles the planes its post steps need with one twk_assemble_devices and runs
  // them on the assembled frame)
  int   tileAssembly = 0;
  // "temporalAccumulation" (1: the batch loop is an orbit of "temporalFrames" frames, each samplesSqrt² iterations from a camera
  // "temporalOrbitStep" of a full turn further in phi, merged into the frames before it by twk_temporal_accumulate — on several
  // devices through twk_render_geometry_tile, twk_assemble_devices_with_geometry and twk_temporal_accumulate_assembled),
  // "temporalMaxHistory", "temporalPositionTolerance" (TwkTemporal; twk_temporal_defaults' values until a key sets them)
  int   temporalAccumulation = 0;
  int   temporalFrames = 1;
  float temporalOrbitStep = TWK_TEMPORAL_ORBIT_STEP;
  int   temporalMaxHistory = TWK_TEMPORAL_MAX_HISTORY;
  float temporalPositionTolerance = TWK_TEMPORAL_POSITION_TOLERANCE;
  // "temporalRectify" (1: that loop merges with twk_temporal_accumulate_rectified / twk_temporal_accumulate_assembled_rectified),
  // "temporalRectifyGamma", "temporalRectifyRadius", "temporalRectifyMinTaps" (TwkTemporalRectify; twk_temporal_rectify_defaults'
  // values until a key sets them); temporalRectifyKeys: how many of the four keys the description holds
  int   temporalRectify = 0;
  float temporalRectifyGamma = TWK_TEMPORAL_RECTIFY_GAMMA;
  int   temporalRectifyRadius = TWK_TEMPORAL_RECTIFY_RADIUS;
  int   temporalRectifyMinTaps = TWK_TEMPORAL_RECTIFY_MIN_TAPS;
  int   temporalRectifyKeys = 0;
  // "temporalInstanceStep <idInstance> <dx> <dy> <dz>" (read by twk_app_get_temporal_motion): before every frame of that loop after
  // the first, the instance is translated by one more step (twk_update_instance_transform on every device). temporalInstance -1: no key.
  int   temporalInstance = -1;
  // "selectiveUpdate 0|1" (read by twk_app_get_selective_update): a render loop sets twk_set_update_mode(TWK_UPDATE_SELECTIVE) on
  // every device before the build, so that the updates of "temporalInstanceStep" rebuild only what the instance changes
  int   selectiveUpdate = 0;
  float temporalInstanceStep[3] = {0.0f, 0.0f, 0.0f};
  // "movingEmitters 0|1" (written back by twk_app_system_description, where a render loop reads it): the loop sets
  // twk_enable_emitter_motion on every device, so that "temporalInstanceStep" may name the instance that carries the light
  int   movingEmitters = 0;
  int   adaptiveSampling = 0;
  int   adaptiveMaxSamples = (int) TWK_ADAPTIVE_MAX_SAMPLES;
  // "adaptiveBudget" (1: each interval of the adaptive loop is one twk_adaptive_plan + one twk_launch_adaptive_planned, every pixel
  // at the samples its own estimate predicts; in effect only with adaptive sampling itself), "adaptiveMinBatch", "adaptiveMaxBatch"
  // (1 <= min <= max <= 64; the provisional defaults of twk_adaptive_plan_defaults)
  int   adaptiveBudget = 0;
  int   adaptiveMinBatch = TWK_DENOISER_MIN_SAMPLES;
  int   adaptiveMaxBatch = 64;
  int   shaderVariant = 0; // grammar extension "shaderVariant": 0 rtigo3, 1 Optix7Gui light-hit rule (include/tweeker_hip.h TWK_SHADERS_*)
  int   samplesSqrt   = 1;
  int   resolution[2] = {1, 1};
  int   tileSize[2]   = {8, 8};
  int   pathLengths[2] = {0, 2};
  float epsilonFactor = 500.0f;
  float envRotation   = 0.0f;
  float clockFactor   = 1000.0f;
  std::string environment;
  std::string prefixScreenshot = "./img";
  TwkTonemapper tonemapper = {1.0f, 1.0f, {1.0f, 1.0f, 1.0f}, 1.0f, 0.0f, 1.0f, 1.0f}; // neutral (Application.cpp:111-120)
  OrbitCamera camera;

  std::vector<TwkCameraDefinition> cameras;
  std::vector<TwkLightDefinition>  lights;
  std::vector<TwkMaterialGUI>      materials;
  std::vector<std::string>         materialNames;
  std::vector<std::shared_ptr<TrianglesNode>> geometries;
  std::vector<FlatInstance>        instances;
  std::vector<std::string>         warnings;

private:
  void createCameras();
  void createLights();
  void appendInstance(std::shared_ptr<TrianglesNode> geometry, const float trafo[12], const std::string& reference);
  void flatten(const std::shared_ptr<SceneNode>& node, const float matrix[12], int material, int light);

  std::shared_ptr<GroupNode>          m_scene;
  std::map<std::string, int>          m_materialReferences;
  std::map<std::string, unsigned int> m_geometryKeys;
};

} // namespace twk

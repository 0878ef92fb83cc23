// rtigo3_hip: command-line front end over libtweeker_hip.so for the batch path of the reference's rtigo3
//   rtigo3 -s system.txt -d scene.txt -m 1
// (main.cpp:169-172 → Application::benchmark, Application.cpp:491-531): render samplesSqrt² iterations, wait for the
// device, print "<iterations> / <seconds> = <fps> fps", store the tonemapped screenshot. Options as Options.cpp:44-156.
// With "targetNoise e" in the system description the loop may end earlier: every "targetNoiseInterval" iterations each device
// estimates the noise of its own buffer (twk_estimate_noise), the summaries are merged, and the loop ends once the
// "targetNoiseQuantile" quantile of the relative standard error is at most e; a second line prints the final mean and quantile.
// With "adaptiveSampling 1" beside it the loop renders uniformly up to the first check only; from then on every device selects the
// pixels above the target (twk_adaptive_select) and renders "targetNoiseInterval" more samples of those alone
// (twk_launch_adaptive) between two checks; with "adaptiveBudget 1" too, each interval is instead one plan (twk_adaptive_plan) and
// one planned pass (twk_launch_adaptive_planned) that gives every selected pixel the samples its own estimate predicts. It ends
// when the target is met, when no device selects anything, or when the samples spent reach the uniform budget, samplesSqrt² x the pixel count; the second line gains the samples per pixel and the active share.
// With "fireflyCascade 1" the accumulate kernels also fold the firefly cascade's layers (twk_enable_cascade); the screenshot is then
// the RESOLVED picture (twk_cascade_resolve), which also stands in as the beauty of whichever denoiser mode is on — guides and
// moments stay the handle's own. The loop, its frame-rate line, the noise estimate and the adaptive passes are what they are
// without it. One device only: refused before any device is created — unless the tiled frame is assembled:
// With "tileAssembly 1", several devices and strategy 3 the guided and sampled-variance denoisers and the cascade are not refused:
// after the loop ONE twk_assemble_devices on the first device assembles exactly the planes those steps need (beauty or cascade
// layers, albedo, normal, moments), and they run on the assembled frame through their explicit forms. With strategy 1 or 2 the key
// is refused (the beauty lives in the shared frame, the other planes do not); on one device it changes nothing.
// With "temporalAccumulation 1" the batch is the loop of a camera that moves (INTEGRATION.md "The temporal seam on several devices"):
// an orbit of "temporalFrames" frames, frame f from the camera at phi + f x "temporalOrbitStep" of a turn under the sample offset
// f x samplesSqrt², each samplesSqrt² iterations, its geometry AOV (twk_render_geometry; twk_render_geometry_tile on several
// devices), there ONE twk_assemble_devices_with_geometry of the planes the merge and the post steps read, and the merge
// (twk_temporal_accumulate; twk_temporal_accumulate_assembled on the first device), the cascade's layers through it with
// "fireflyCascade 1". After the last frame the merged layers are resolved, the denoiser takes the merged colour (or the resolved
// picture) and the merged moments, and the screenshot is that. The frame-rate line counts frames x samplesSqrt² iterations.
// Refused before any device is created: with "targetNoise" or "adaptiveSampling", with a "lensShader" other than 0, with strategy 1
// or 2, and on several devices without "tileAssembly 1". With "temporalRectify 1" beside it the merge is the rectified one
// (twk_temporal_accumulate_rectified; twk_temporal_accumulate_assembled_rectified on the first device) with "temporalRectifyGamma",
// "temporalRectifyRadius" and "temporalRectifyMinTaps"; any of these four keys without "temporalAccumulation 1" is refused before any
// device is created. With "temporalInstanceStep <idInstance> <dx> <dy> <dz>" beside it that instance is translated by one more step
// before every frame after the first (twk_update_instance_transform on every device, which keeps the history; the merges carry it
// along); refused before any device is created without "temporalAccumulation 1", for an id beyond the scene's instances and for an
// instance that carries a light — unless "movingEmitters 1" stands beside it: then twk_enable_emitter_motion is set on every device
// before the loop and the light's definition moves with its instance (include/tweeker_hip.h "Moving a light").
// With "denoiserGeometry 1" beside "denoiser 3" the filter, in whichever mode is on, is twk_denoise_geometry: the geometry AOV is
// traced once before the screenshot is filtered (twk_render_geometry; on several devices with "tileAssembly 1"
// twk_render_geometry_tile and ONE twk_assemble_devices_with_geometry), the temporal loop uses its last frame's own geometry, and
// the camera is the first device's camera 0. Refused before any device is created: a "lensShader" other than 0, a scene with
// cutout opacity, and several devices without an assembled frame.
// The interactive mode (-m 0: GLFW window, imgui) needs a display and is not part of this build.
//
// Multi-GPU: `strategy` > 0 in the system description renders with every visible device selected by `devicesMask`
// (Raytracer.cpp:60-123), each device its checkerboard share into a local buffer (DeviceMultiGPULocalCopy.cpp), then
// ONE peer copy per device and ONE compositor launch on the first device. TWK_CLI_VIRTUAL_DEVICES=N shares one
// physical GPU between N handles (testing on a single-GPU machine).
#include "tweeker_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {

struct Options // Options.cpp:33-38 defaults
{
  int width = 512, height = 512, mode = 0;
  std::string system, scene;
};

void printUsage(const std::string& argv0)
{
  std::cerr << "\nUsage: " << argv0 << " [options]\n"
            << "App Options:\n"
               "   ? | help | --help       Print this usage message and exit.\n"
               "  -w | --width <int>       Width of the client window  (512), unused without a display\n"
               "  -h | --height <int>      Height of the client window (512), unused without a display\n"
               "  -m | --mode <int>        0 = interactive (not available in this build), 1 == benchmark (0)\n"
               "  -s | --system <filename> Filename for system options (empty).\n"
               "  -d | --desc   <filename> Filename for scene description (empty).\n"
            << std::endl;
}

bool parseCommandLine(int argc, char* argv[], Options& o)
{
  for (int i = 1; i < argc; ++i)
  {
    const std::string arg(argv[i]);
    if (arg == "?" || arg == "help" || arg == "--help") { printUsage(argv[0]); return false; }
    const bool known = arg == "-w" || arg == "--width" || arg == "-h" || arg == "--height" || arg == "-m" || arg == "--mode" ||
                       arg == "-s" || arg == "--system" || arg == "-d" || arg == "--desc";
    if (!known) { std::cerr << "Unknown option '" << arg << "'\n"; printUsage(argv[0]); return false; }
    if (i == argc - 1) { std::cerr << "Option '" << arg << "' requires additional argument.\n"; printUsage(argv[0]); return false; }
    const char* value = argv[++i];
    if      (arg == "-w" || arg == "--width")  o.width  = atoi(value);
    else if (arg == "-h" || arg == "--height") o.height = atoi(value);
    else if (arg == "-m" || arg == "--mode")   o.mode   = atoi(value);
    else if (arg == "-s" || arg == "--system") o.system = value;
    else                                       o.scene  = value;
  }
  return true;
}

// ≙ Application::createPictures (Application.cpp:679-699) + Raytracer::initTextures: the two hard-coded material
// pictures and, for miss 2, the environment map named by "envMap". A picture that cannot be read is reported and
// skipped (materials that ask for it then render untextured); a progressive JPEG is not decodable here, so the
// albedo picture is also looked up as ./NVIDIA_Logo.png.
struct PictureFile { int slot; std::vector<std::string> candidates; };

bool loadPicture(const PictureFile& picture, int& width, int& height, std::vector<float>& rgba)
{
  for (const std::string& path : picture.candidates)
  {
    if (twk_load_image(path.c_str(), &width, &height, nullptr, 0) != TWK_SUCCESS) continue;
    rgba.resize((size_t) width * height * 4);
    if (twk_load_image(path.c_str(), &width, &height, rgba.data(), rgba.size()) == TWK_SUCCESS)
    {
      std::cerr << "INFO: picture " << path << " " << width << " x " << height << std::endl;
      return true;
    }
  }
  std::cerr << "WARNING: picture " << picture.candidates.front() << " not loaded: " << twk_last_error() << std::endl;
  return false;
}

#define TWK_OK(call) do { if ((call) != TWK_SUCCESS) { std::cerr << "ERROR: " << #call << ": " << twk_last_error() << std::endl; return 1; } } while (0)
#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::cerr << "ERROR: " << #call << ": " << hipGetErrorString(e_) << std::endl; return 1; } } while (0)

} // namespace

int main(int argc, char* argv[])
{
  Options options;
  if (!parseCommandLine(argc, argv, options)) return 1;
  if (options.system.empty() || options.scene.empty())
  {
    std::cerr << "ERROR: system (-s) and scene (-d) description files are required.\n";
    printUsage(argv[0]);
    return 1;
  }
  if (std::max(0, options.mode) != 1)
  {
    std::cerr << "ERROR: mode 0 (interactive) needs a GLFW window; this build runs the benchmark mode only: -m 1\n";
    return 1;
  }

  TwkApp app = nullptr;
  TWK_OK(twk_app_create(&app, options.system.c_str(), options.scene.c_str()));
  TwkAppInfo info;
  TWK_OK(twk_app_info(app, &info));

  // device selection (Raytracer.cpp:60-123): strategy 0 = first visible device, otherwise all visible devices in the mask
  int visible = 0;
  TWK_OK(twk_device_count(&visible));
  std::vector<int> ordinals;
  const char* virtualDevices = getenv("TWK_CLI_VIRTUAL_DEVICES");
  if (info.strategy == 0) ordinals.push_back(0);
  else if (virtualDevices && atoi(virtualDevices) > 0) ordinals.assign((size_t) std::min(32, atoi(virtualDevices)), 0);
  else
  {
    for (int d = 0; d < visible && d < 32; ++d) if (info.devicesMask & (1 << d)) ordinals.push_back(d);
  }
  if (ordinals.empty()) { std::cerr << "ERROR: no device selected by devicesMask " << info.devicesMask << " (" << visible << " visible)\n"; return 1; }
  const int count = (int) ordinals.size();

  // "denoiser" on: the picture is the tonemapped DENOISED image, as Optix7Gui displays it (optixDenoiserInvoke, then the
  // texture, Application.cpp:942-1001), filtered after the benchmark line: the frame rate is the renderer's. The guides are the
  // AOVs of ONE device (they are packed tile buffers on several and are not assembled): decided here, before any GPU work.
  int denoiserEnabled = 0;
  TwkDenoiser denoiser;
  TWK_OK(twk_app_get_denoiser(app, &denoiserEnabled, &denoiser));
  int denoiserVarianceEnabled = 0; // "denoiserVariance 1": the variance-guided, firefly-clamping mode of the filter
  TwkDenoiserVariance denoiserVariance;
  TWK_OK(twk_app_get_denoiser_variance(app, &denoiserVarianceEnabled, &denoiserVariance));
  int denoiserSampledEnabled = 0, denoiserMinSamples = 0; // "denoiserSampledVariance 1": the measured variance of the samples guides the filter
  TWK_OK(twk_app_get_denoiser_sampled(app, &denoiserSampledEnabled, &denoiserMinSamples));
  int tileAssembly = 0; // "tileAssembly 1": the planes the post steps need are assembled on the first device (strategy 3)
  TWK_OK(twk_app_get_tile_assembly(app, &tileAssembly));
  if (tileAssembly && count > 1 && (info.strategy == 1 || info.strategy == 2))
  {
    std::cerr << "ERROR: tileAssembly assembles packed tile buffers (strategy 3); with strategy 1 or 2 the beauty lives in a shared frame and the other planes do not\n";
    return 1;
  }
  const bool assembling = tileAssembly && count > 1 && info.strategy == 3;
  // "denoiserGeometry 1" beside "denoiser 3": the filter's fourth guide is the geometry AOV (twk_denoise_geometry), traced once
  // before the screenshot is filtered. What the geometry AOV refuses is refused here, before any device is created.
  int denoiserGeometryKey = 0;
  TwkDenoiserGeometry denoiserGeometry;
  TWK_OK(twk_app_get_denoiser_geometry(app, &denoiserGeometryKey, &denoiserGeometry));
  const bool geometryGuide = denoiserEnabled && denoiserGeometryKey && denoiser.inputKind == TWK_DENOISER_RGB_ALBEDO_NORMAL;
  if (geometryGuide && info.lensShader != 0)
  {
    std::cerr << "ERROR: denoiserGeometry reads the geometry AOV, which is traced through the pinhole camera: lensShader must be 0\n";
    return 1;
  }
  if (geometryGuide && count > 1 && !assembling)
  {
    std::cerr << "ERROR: denoiserGeometry on several devices reads the assembled geometry AOV on the first device: it needs tileAssembly 1 (strategy 3)\n";
    return 1;
  }
  if (geometryGuide)
  {
    std::vector<TwkMaterialGUI> materials((size_t) std::max(1, info.numMaterials));
    TWK_OK(twk_app_get_materials(app, materials.data(), (int) materials.size()));
    for (int m = 0; m < info.numMaterials; ++m)
      if (materials[(size_t) m].useCutoutTexture)
      {
        std::cerr << "ERROR: denoiserGeometry reads the geometry AOV, a geometric query: not for scenes with cutout opacity\n";
        return 1;
      }
  }
  if (denoiserEnabled && denoiserSampledEnabled && count > 1 && !assembling)
  {
    std::cerr << "ERROR: denoiserSampledVariance needs the luminance moments of ONE device; they are packed tile buffers on several and are not assembled\n";
    return 1;
  }
  if (denoiserEnabled && count > 1 && denoiser.inputKind != TWK_DENOISER_RGB && !assembling)
  {
    std::cerr << "ERROR: denoiser " << denoiser.inputKind + 1 << " needs the albedo / normal AOVs of ONE device; with several devices only denoiser 1 (no guides) filters the assembled frame\n";
    return 1;
  }

  int targetNoiseEnabled = 0, targetNoiseInterval = 0; // "targetNoise e": the stopping rule
  float targetNoise = 0.0f, targetNoiseQuantile = 0.0f;
  TWK_OK(twk_app_get_target_noise(app, &targetNoiseEnabled, &targetNoise, &targetNoiseQuantile, &targetNoiseInterval));

  int adaptiveEnabled = 0; // "adaptiveSampling 1": between the checks only the pixels above the target are sampled
  TwkAdaptive adaptive;
  TWK_OK(twk_app_get_adaptive(app, &adaptiveEnabled, &adaptive));
  if (adaptiveEnabled && count > 1 && (info.strategy == 1 || info.strategy == 2))
  {
    std::cerr << "ERROR: adaptiveSampling renders into packed tile buffers (strategy 0 or 3), not into a shared frame (strategy 1 or 2)\n";
    return 1;
  }

  int planEnabled = 0; // "adaptiveBudget 1": each interval is one plan + one planned pass, every pixel at the samples its estimate predicts
  TwkAdaptivePlan adaptivePlan;
  TWK_OK(twk_app_get_adaptive_plan(app, &planEnabled, &adaptivePlan));

  int cascadeEnabled = 0; // "fireflyCascade 1": the screenshot is the cascade's resolved picture
  TwkCascade cascade;
  TwkCascadeResolve cascadeResolve;
  TWK_OK(twk_app_get_cascade(app, &cascadeEnabled, &cascade, &cascadeResolve));
  if (cascadeEnabled && count > 1 && !assembling)
  {
    std::cerr << "ERROR: fireflyCascade resolves the layers of ONE device; they are packed tile buffers on several and are not assembled\n";
    return 1;
  }

  int temporalEnabled = 0, temporalFrames = 1; // "temporalAccumulation 1": the batch is an orbit of merged frames
  float temporalOrbitStep = 0.0f;
  TwkTemporal temporal;
  TWK_OK(twk_app_get_temporal(app, &temporalEnabled, &temporal, &temporalFrames, &temporalOrbitStep));
  int rectifyEnabled = 0, rectifyKeys = 0; // "temporalRectify 1": the orbit's merge is the rectified one
  TwkTemporalRectify rectify;
  TWK_OK(twk_app_get_temporal_rectify(app, &rectifyEnabled, &rectify, &rectifyKeys));
  if (rectifyKeys > 0 && !temporalEnabled)
  {
    std::cerr << "ERROR: temporalRectify, temporalRectifyGamma, temporalRectifyRadius and temporalRectifyMinTaps set the merge of the moving-camera loop: they need temporalAccumulation 1\n";
    return 1;
  }
  int movingInstance = -1; // "temporalInstanceStep": an instance translated by one more step before every frame after the first
  float movingStep[3] = {0.0f, 0.0f, 0.0f};
  TWK_OK(twk_app_get_temporal_motion(app, &movingInstance, movingStep));
  if (movingInstance >= 0 && !temporalEnabled)
  {
    std::cerr << "ERROR: temporalInstanceStep moves an object in the moving-camera loop: it needs temporalAccumulation 1\n";
    return 1;
  }
  // "movingEmitters 1": read where the application writes its settings back, in the loader's own grammar (a key on a line of its own)
  bool movingEmitters = false;
  {
    size_t length = 0;
    TWK_OK(twk_app_system_description(app, nullptr, 0, &length));
    std::vector<char> text(length + 1, 0);
    TWK_OK(twk_app_system_description(app, text.data(), text.size(), nullptr));
    std::istringstream lines(text.data());
    for (std::string line; std::getline(lines, line);) if (line == "movingEmitters 1") movingEmitters = true;
  }
  if (movingInstance >= 0)
  {
    int light = -1;
    if (movingInstance >= info.numInstances || twk_app_get_instance(app, movingInstance, nullptr, nullptr, nullptr, &light) != TWK_SUCCESS)
    {
      std::cerr << "ERROR: temporalInstanceStep names instance " << movingInstance << "; the scene has " << info.numInstances << "\n";
      return 1;
    }
    if (light >= 0 && !movingEmitters)
    {
      std::cerr << "ERROR: temporalInstanceStep names an instance that carries a light: moving emitters is not supported\n";
      return 1;
    }
  }
  if (temporalEnabled && (targetNoiseEnabled || adaptiveEnabled))
  {
    std::cerr << "ERROR: temporalAccumulation renders a fixed orbit of frames; targetNoise and adaptiveSampling end or thin a single frame's loop and do not go with it\n";
    return 1;
  }
  if (temporalEnabled && info.lensShader != 0)
  {
    std::cerr << "ERROR: temporalAccumulation reprojects through the pinhole camera: lensShader must be 0\n";
    return 1;
  }
  if (temporalEnabled && count > 1 && (info.strategy == 1 || info.strategy == 2))
  {
    std::cerr << "ERROR: temporalAccumulation on several devices merges the assembled packed tile buffers (strategy 3), not a shared frame (strategy 1 or 2)\n";
    return 1;
  }
  if (temporalEnabled && count > 1 && !assembling)
  {
    std::cerr << "ERROR: temporalAccumulation on several devices merges the assembled frame on the first device: it needs tileAssembly 1\n";
    return 1;
  }

  std::vector<TwkDevice> devices((size_t) count, nullptr);
  TwkDeviceState state;
  TWK_OK(twk_app_get_state(app, &state));
  for (int i = 0; i < count; ++i) TWK_OK(twk_device_create(&devices[(size_t) i], ordinals[(size_t) i], i, count, info.miss));

  std::vector<PictureFile> pictures = {{TWK_TEXTURE_ALBEDO, {"./NVIDIA_Logo.jpg", "./NVIDIA_Logo.png"}}, {TWK_TEXTURE_CUTOUT, {"./slots_alpha.png"}}};
  char environment[4096];
  TWK_OK(twk_app_get_environment(app, environment, sizeof(environment)));
  if (info.miss == 2 && environment[0] != 0) pictures.push_back({TWK_TEXTURE_ENVIRONMENT, {environment}});
  for (const PictureFile& picture : pictures)
  {
    int w = 0, h = 0;
    std::vector<float> rgba;
    if (!loadPicture(picture, w, h, rgba)) continue;
    for (int i = 0; i < count; ++i) TWK_OK(twk_init_texture(devices[(size_t) i], picture.slot, rgba.data(), w, h));
  }
  // "selectiveUpdate 1": the mode is read by the build, so it is set before the scene is handed over
  int selectiveUpdate = 0;
  TWK_OK(twk_app_get_selective_update(app, &selectiveUpdate));
  if (selectiveUpdate)
    for (int i = 0; i < count; ++i) TWK_OK(twk_set_update_mode(devices[(size_t) i], TWK_UPDATE_SELECTIVE));
  for (int i = 0; i < count; ++i) TWK_OK(twk_app_init_device(app, devices[(size_t) i]));
  if (movingEmitters)
    for (int i = 0; i < count; ++i) TWK_OK(twk_enable_emitter_motion(devices[(size_t) i], 1));

  // Buffer strategy (Raytracer.cpp:125-176 picks the Device flavour): 1 = zero copy — one pinned host frame mapped into
  // every device (DeviceMultiGPUZeroCopy.cpp:106-118); 2 = peer access — one frame on the first device, written by its
  // peers (DeviceMultiGPUPeerAccess.cpp:110-158); 3 = local copy — packed tile buffers + compositor.
  // "outputFormat 1" (≙ Optix7Gui USE_FP32_OUTPUT 0): every buffer below holds RGBA16F, 8 bytes per pixel
  int outputFormat = TWK_OUTPUT_FLOAT4;
  TWK_OK(twk_app_get_output_format(app, &outputFormat));
  const bool half = (outputFormat == TWK_OUTPUT_HALF4);
  const size_t pixelBytes = half ? 8 : 16;
  void* sharedFrame = nullptr;
  const size_t frameBytes = (size_t) info.resolution[0] * info.resolution[1] * pixelBytes;
  if (count > 1 && info.strategy == 1)
  {
    HIP_OK(hipHostMalloc(&sharedFrame, frameBytes, hipHostMallocPortable | hipHostMallocMapped));
    memset(sharedFrame, 0, frameBytes);
  }
  else if (count > 1 && info.strategy == 2)
  {
    HIP_OK(hipSetDevice(ordinals[0]));
    HIP_OK(hipMalloc(&sharedFrame, frameBytes));
    HIP_OK(hipMemset(sharedFrame, 0, frameBytes));
    for (int i = 1; i < count; ++i)
    {
      if (ordinals[(size_t) i] == ordinals[0]) continue;
      int canAccess = 0;
      HIP_OK(hipDeviceCanAccessPeer(&canAccess, ordinals[(size_t) i], ordinals[0]));
      if (!canAccess) { std::cerr << "ERROR: device " << ordinals[(size_t) i] << " cannot access the frame on device " << ordinals[0] << " (strategy 2 needs one peer-to-peer island)\n"; return 1; }
      HIP_OK(hipSetDevice(ordinals[(size_t) i]));
      const hipError_t e = hipDeviceEnablePeerAccess(ordinals[0], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { std::cerr << "ERROR: hipDeviceEnablePeerAccess: " << hipGetErrorString(e) << std::endl; return 1; }
      (void) hipGetLastError();
    }
  }
  if (sharedFrame) for (int i = 0; i < count; ++i) TWK_OK(twk_set_shared_frame(devices[(size_t) i], sharedFrame, frameBytes));
  std::cerr << "INFO: " << count << " device(s), " << info.resolution[0] << " x " << info.resolution[1] << ", "
            << info.samplesSqrt * info.samplesSqrt << " spp, " << info.numInstances << " instances" << std::endl;

  // Application::benchmark (Application.cpp:491-513)
  const unsigned int spp = (unsigned int) (info.samplesSqrt * info.samplesSqrt);
  const auto start = std::chrono::steady_clock::now();
  unsigned int iterationIndex = 0;
  TwkNoiseSummary noise;
  memset(&noise, 0, sizeof(noise));
  float noiseQuantile = 0.0f;
  bool noiseChecked = false; // `noise` is the summary of the frame as it stands
  bool adaptivePhase = false; // the first check has not met the target and "adaptiveSampling" is on
  // every device estimates its own buffer (a packed tile buffer's padding is empty), the host merges; true: the target is met
  auto checkNoise = [&](bool& met) -> int
  {
    memset(&noise, 0, sizeof(noise));
    for (int i = 0; i < count; ++i) TWK_OK(twk_estimate_noise(devices[(size_t) i], nullptr, nullptr, 0, nullptr));
    for (int i = 0; i < count; ++i)
    {
      TwkNoiseSummary part;
      TWK_OK(twk_read_noise(devices[(size_t) i], &part));
      TWK_OK(twk_noise_merge(&noise, &part));
    }
    met = false;
    if (noise.valid > 0)
    {
      TWK_OK(twk_noise_quantile(&noise, targetNoiseQuantile, &noiseQuantile));
      met = (noiseQuantile <= targetNoise);
    }
    return 0;
  };
  // the planes the temporal loop's assembly moves beside the geometry: what the merge reads and, of the last frame, the post steps' guides
  unsigned int temporalPlanes = TWK_PLANE_BIT(TWK_PLANE_OUTPUT) | TWK_PLANE_BIT(TWK_PLANE_MOMENTS);
  if (cascadeEnabled) temporalPlanes |= TWK_PLANE_BIT(TWK_PLANE_CASCADE);
  if (temporalEnabled)
  {
    if (cascadeEnabled) TWK_OK(twk_temporal_enable_cascade(devices[0], 1));
    const float aspect = (float) ((double) info.resolution[0] / (double) info.resolution[1]);
    for (int frame = 0; frame < temporalFrames; ++frame)
    {
      TwkCameraDefinition camera;
      const float phi = (float) ((double) info.phi + (double) frame * (double) temporalOrbitStep);
      TWK_OK(twk_camera_frustum(info.center, phi, info.theta, info.fov, info.distance, aspect, &camera));
      if (movingInstance >= 0 && frame > 0)
        for (int i = 0; i < count; ++i)
        {
          float transform[12];
          TWK_OK(twk_get_instance_transform(devices[(size_t) i], movingInstance, transform));
          for (int k = 0; k < 3; ++k) transform[4 * k + 3] += movingStep[k];
          TWK_OK(twk_update_instance_transform(devices[(size_t) i], movingInstance, transform));
          // which path the update took and what it touched, per device: the only way to see from outside that "selectiveUpdate 1" took effect
          TwkUpdateInfo update;
          TWK_OK(twk_get_update_info(devices[(size_t) i], &update));
          std::cerr << "INFO: frame " << frame << ", device " << i << ": instance " << movingInstance << " moved by a " << (update.selective ? "selective" : "full") << " update, "
                    << update.treesRebuilt << " tree(s) rebuilt, " << update.nodesRequantised << " node(s) requantised" << std::endl;
        }
      for (int i = 0; i < count; ++i)
      {
        TWK_OK(twk_update_camera(devices[(size_t) i], 0, &camera));
        TWK_OK(twk_set_sample_offset(devices[(size_t) i], (unsigned int) frame * spp));
      }
      for (unsigned int it = 0; it < spp; ++it) for (int i = 0; i < count; ++i) TWK_OK(twk_launch(devices[(size_t) i], it));
      if (count == 1)
      {
        TWK_OK(twk_render_geometry(devices[0]));
        if (rectifyEnabled) TWK_OK(twk_temporal_accumulate_rectified(devices[0], &temporal, &rectify, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr));
        else                TWK_OK(twk_temporal_accumulate(devices[0], &temporal, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr));
        continue;
      }
      for (int i = 0; i < count; ++i) TWK_OK(twk_render_geometry_tile(devices[(size_t) i]));
      unsigned int planes = temporalPlanes;
      if (frame == temporalFrames - 1 && denoiserEnabled && denoiser.inputKind >= TWK_DENOISER_RGB_ALBEDO) planes |= TWK_PLANE_BIT(TWK_PLANE_ALBEDO);
      if (frame == temporalFrames - 1 && denoiserEnabled && denoiser.inputKind >= TWK_DENOISER_RGB_ALBEDO_NORMAL) planes |= TWK_PLANE_BIT(TWK_PLANE_NORMAL);
      TWK_OK(twk_assemble_devices_with_geometry(devices[0], planes, devices.data(), count));
      if (rectifyEnabled) TWK_OK(twk_temporal_accumulate_assembled_rectified(devices[0], &temporal, &rectify));
      else                TWK_OK(twk_temporal_accumulate_assembled(devices[0], &temporal));
    }
    iterationIndex = (unsigned int) temporalFrames * spp;
  }
  while (iterationIndex < spp)
  {
    for (int i = 0; i < count; ++i) TWK_OK(twk_launch(devices[(size_t) i], iterationIndex));
    ++iterationIndex;
    noiseChecked = false;
    if (targetNoiseEnabled && iterationIndex % (unsigned int) targetNoiseInterval == 0)
    {
      bool met = false;
      if (checkNoise(met)) return 1;
      noiseChecked = true;
      if (met) break;
      if (adaptiveEnabled) { adaptivePhase = true; break; }
    }
  }
  // The adaptive loop (INTEGRATION.md "The adaptive loop"): select, render the interval's samples on the selected pixels, check
  const unsigned long long pixelCount = (unsigned long long) info.resolution[0] * (unsigned long long) info.resolution[1];
  const unsigned long long budget = (unsigned long long) spp * pixelCount;
  unsigned long long spent = (unsigned long long) iterationIndex * pixelCount, lastActive = pixelCount;
  const char* adaptiveEnd = "target met";
  if (adaptivePhase)
  {
    int batch = 64; // samples per pass at most: the launch batch (TWK_BATCH, as the handles read it)
    if (const char* e = getenv("TWK_BATCH")) batch = std::max(1, std::min(64, atoi(e)));
    std::vector<unsigned int> numActive((size_t) count, 0u);
    for (;;)
    {
      if (planEnabled)
      {
        // every device plans its own packed tile buffer (the padding is empty: budget 0); when the plans together ask for more than
        // the budget has left, every selected pixel gets the same share of what is left instead, as in the fixed loop below
        TwkAdaptivePlan plan = adaptivePlan;
        unsigned long long paths = 0;
        for (int attempt = 0; attempt < 2; ++attempt)
        {
          lastActive = 0; paths = 0;
          for (int i = 0; i < count; ++i)
          {
            unsigned long long numPaths = 0;
            TWK_OK(twk_adaptive_plan(devices[(size_t) i], &adaptive, &plan, nullptr, nullptr, 0, nullptr, nullptr, &numActive[(size_t) i], &numPaths));
            lastActive += numActive[(size_t) i]; paths += numPaths;
          }
          if (lastActive == 0 || paths <= budget - spent) break;
          const unsigned long long share = std::min<unsigned long long>((budget - spent) / lastActive, (unsigned long long) adaptivePlan.maxBatch);
          if (share == 0) { paths = 0; break; }
          plan.minBatch = plan.maxBatch = (uint32_t) share;
        }
        if (lastActive == 0) { adaptiveEnd = "nothing selected"; break; }
        if (paths == 0 || paths > budget - spent) { adaptiveEnd = "budget spent"; break; }
        for (int i = 0; i < count; ++i) TWK_OK(twk_launch_adaptive_planned(devices[(size_t) i]));
        spent += paths;
        bool met = false;
        if (checkNoise(met)) return 1;
        if (met) break;
        continue;
      }
      lastActive = 0;
      for (int i = 0; i < count; ++i)
      {
        TWK_OK(twk_adaptive_select(devices[(size_t) i], &adaptive, nullptr, nullptr, 0, nullptr, &numActive[(size_t) i]));
        lastActive += numActive[(size_t) i];
      }
      if (lastActive == 0) { adaptiveEnd = "nothing selected"; break; }
      unsigned long long left = std::min<unsigned long long>((unsigned long long) targetNoiseInterval, (budget - spent) / lastActive);
      if (left == 0) { adaptiveEnd = "budget spent"; break; }
      while (left > 0)
      {
        const int samples = (int) std::min<unsigned long long>(left, (unsigned long long) batch);
        for (int i = 0; i < count; ++i) TWK_OK(twk_launch_adaptive(devices[(size_t) i], samples));
        spent += lastActive * (unsigned long long) samples;
        left -= (unsigned long long) samples;
      }
      bool met = false;
      if (checkNoise(met)) return 1;
      if (met) break;
    }
    noiseChecked = true; // nothing was rendered after the last check
    iterationIndex = (unsigned int) ((spent + pixelCount - 1) / pixelCount); // the mean samples per pixel, rounded up
  }
  for (int i = 0; i < count; ++i) TWK_OK(twk_sync(devices[(size_t) i]));
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
  const double fps = double(iterationIndex) / seconds;
  {
    std::ostringstream stream;
    stream.precision(3);
    stream << std::fixed << iterationIndex << " / " << seconds << " = " << fps << " fps";
    std::cout << stream.str() << std::endl;
  }
  if (targetNoiseEnabled)
  {
    bool met = false;
    if (!noiseChecked && checkNoise(met)) return 1; // samplesSqrt² is no multiple of the interval: the frame's own figures
    std::ostringstream stream;
    stream << "noise: " << iterationIndex << " spp";
    if (noise.valid > 0)
    {
      float mean = 0.0f;
      TWK_OK(twk_noise_mean(&noise, &mean));
      stream << ", mean " << mean << ", " << targetNoiseQuantile << " quantile at most " << noiseQuantile << ", target " << targetNoise;
    }
    else stream << ", no pixel has enough samples yet, target " << targetNoise;
    if (adaptivePhase)
    {
      unsigned int largest = 0;
      for (int i = 0; i < count; ++i)
      {
        int launchWidth = 0;
        TWK_OK(twk_get_launch_width(devices[(size_t) i], &launchWidth));
        std::vector<uint32_t> counts((size_t) launchWidth * (size_t) info.resolution[1]);
        TWK_OK(twk_read_sample_counts(devices[(size_t) i], counts.data(), counts.size()));
        for (const uint32_t c : counts) largest = std::max(largest, (unsigned int) c);
      }
      stream << ", adaptive: mean " << double(spent) / double(pixelCount) << " spp, max " << largest << " spp, last active share "
             << double(lastActive) / double(pixelCount) << ", samples " << spent << " of " << budget << ", ended: " << adaptiveEnd;
    }
    std::cout << stream.str() << std::endl;
  }

  // screenshot(true) (Application.cpp:525,2231-2335)
  const int width = info.resolution[0], height = info.resolution[1];
  const size_t numPixels = (size_t) width * height;
  TwkTonemapper tonemapper;
  TWK_OK(twk_app_get_tonemapper(app, &tonemapper));
  std::vector<unsigned char> rgb8(numPixels * 3);
  // tonemaps `frame` (device memory in the output format on the first device; NULL: the first device's own buffers), denoised
  // first when the description asks for it; albedo, normal, moments: the guides beside an explicit frame that has them (the cascade's)
  // geometry: the geometry AOV beside an explicit frame ("denoiserGeometry 1"; its camera is the first device's camera 0)
  auto present = [&](const void* frame, const void* albedo = nullptr, const void* normal = nullptr, const void* moments = nullptr, const void* geometry = nullptr) -> int
  {
    if (denoiserEnabled)
    {
      if (geometryGuide)
        TWK_OK(twk_denoise_geometry(devices[0], &denoiser, &denoiserGeometry, (denoiserSampledEnabled || denoiserVarianceEnabled) ? &denoiserVariance : nullptr,
                                    denoiserSampledEnabled ? denoiserMinSamples : 0, frame, albedo, normal, denoiserSampledEnabled ? moments : nullptr, geometry, nullptr, width, height, nullptr));
      else if (denoiserSampledEnabled)       TWK_OK(twk_denoise_variance_sampled(devices[0], &denoiser, &denoiserVariance, denoiserMinSamples, frame, albedo, normal, moments, width, height, nullptr)); // one device: frame is NULL, the handle's own buffers and moments
      else if (denoiserVarianceEnabled) TWK_OK(twk_denoise_variance(devices[0], &denoiser, &denoiserVariance, frame, albedo, normal, width, height, nullptr));
      else                              TWK_OK(twk_denoise(devices[0], &denoiser, frame, albedo, normal, width, height, nullptr));
      void* denoised = nullptr;
      TWK_OK(twk_get_denoised_device_pointer(devices[0], &denoised, nullptr));
      frame = denoised;
    }
    if (!frame)    TWK_OK(twk_tonemap(devices[0], &tonemapper, nullptr, numPixels, rgb8.data())); // the handle's buffer, in its format
    else if (half) TWK_OK(twk_tonemap_half(devices[0], &tonemapper, frame, numPixels, rgb8.data()));
    else           TWK_OK(twk_tonemap(devices[0], &tonemapper, frame, numPixels, rgb8.data()));
    return 0;
  };
  if (temporalEnabled)
  {
    // the merged colour (with the cascade: the resolve of the merged layers) and the merged moments of the first device; the guides
    // are the last frame's: assembled with it on several devices, copies of the handle's own AOVs on one
    void* merged = nullptr; void* mergedMoments = nullptr; void* resolved = nullptr;
    TWK_OK(twk_get_temporal_device_pointers(devices[0], &merged, nullptr, &mergedMoments, nullptr));
    HIP_OK(hipSetDevice(ordinals[0]));
    if (cascadeEnabled)
    {
      void* layers = nullptr;
      TWK_OK(twk_get_temporal_cascade_device_pointer(devices[0], &layers, nullptr));
      HIP_OK(hipMalloc(&resolved, numPixels * pixelBytes));
      TWK_OK(twk_cascade_resolve(devices[0], &cascade, &cascadeResolve, layers, width, height, resolved));
      merged = resolved;
    }
    void* guides[2] = {nullptr, nullptr}; bool ownGuides = false;
    if (denoiserEnabled && denoiser.inputKind != TWK_DENOISER_RGB)
    {
      if (count > 1)
      {
        TWK_OK(twk_get_assembled_device_pointer(devices[0], TWK_PLANE_ALBEDO, &guides[0], nullptr));
        if (denoiser.inputKind >= TWK_DENOISER_RGB_ALBEDO_NORMAL) TWK_OK(twk_get_assembled_device_pointer(devices[0], TWK_PLANE_NORMAL, &guides[1], nullptr));
      }
      else
      {
        ownGuides = true;
        std::vector<unsigned char> host(numPixels * pixelBytes);
        for (int which = 0; which < 2; ++which)
        {
          TWK_OK(twk_read_aov_raw(devices[0], which == 0 ? TWK_AOV_ALBEDO : TWK_AOV_NORMAL, host.data(), host.size()));
          HIP_OK(hipMalloc(&guides[which], host.size()));
          HIP_OK(hipMemcpy(guides[which], host.data(), host.size(), hipMemcpyHostToDevice));
        }
      }
    }
    void* frameGeometry = nullptr; // the last frame's own geometry: assembled on several devices, the handle's on one
    if (geometryGuide)
    {
      if (count > 1) TWK_OK(twk_get_assembled_geometry_device_pointer(devices[0], &frameGeometry, nullptr));
      else           TWK_OK(twk_get_geometry_device_pointer(devices[0], &frameGeometry, nullptr));
    }
    const int failed = present(merged, guides[0], guides[1], (denoiserEnabled && denoiserSampledEnabled) ? mergedMoments : nullptr, frameGeometry);
    if (ownGuides) for (void* guide : guides) if (guide) HIP_OK(hipFree(guide));
    if (resolved) HIP_OK(hipFree(resolved));
    if (failed) return 1;
  }
  else if (assembling)
  {
    // several devices, packed tile buffers: one assembly of exactly the planes the post steps read, then their explicit forms on
    // the assembled pointers (ordered on the first device's stream; no host round trip, no per-plane gather)
    unsigned int planes = TWK_PLANE_BIT(cascadeEnabled ? TWK_PLANE_CASCADE : TWK_PLANE_OUTPUT);
    if (denoiserEnabled && denoiser.inputKind >= TWK_DENOISER_RGB_ALBEDO) planes |= TWK_PLANE_BIT(TWK_PLANE_ALBEDO);
    if (denoiserEnabled && denoiser.inputKind >= TWK_DENOISER_RGB_ALBEDO_NORMAL) planes |= TWK_PLANE_BIT(TWK_PLANE_NORMAL);
    if (denoiserEnabled && denoiserSampledEnabled) planes |= TWK_PLANE_BIT(TWK_PLANE_MOMENTS);
    void* assembledGeometry = nullptr;
    if (geometryGuide)
    {
      for (int i = 0; i < count; ++i) TWK_OK(twk_render_geometry_tile(devices[(size_t) i]));
      TWK_OK(twk_assemble_devices_with_geometry(devices[0], planes, devices.data(), count));
      TWK_OK(twk_get_assembled_geometry_device_pointer(devices[0], &assembledGeometry, nullptr));
    }
    else TWK_OK(twk_assemble_devices(devices[0], planes, devices.data(), count));
    void* assembled[TWK_PLANE_COUNT] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int p = 0; p < TWK_PLANE_COUNT; ++p) if (planes & TWK_PLANE_BIT(p)) TWK_OK(twk_get_assembled_device_pointer(devices[0], p, &assembled[p], nullptr));
    void* frame = assembled[TWK_PLANE_OUTPUT]; void* resolved = nullptr;
    if (cascadeEnabled)
    {
      HIP_OK(hipSetDevice(ordinals[0]));
      HIP_OK(hipMalloc(&resolved, numPixels * pixelBytes));
      TWK_OK(twk_cascade_resolve(devices[0], &cascade, &cascadeResolve, assembled[TWK_PLANE_CASCADE], width, height, resolved));
      frame = resolved;
    }
    const int failed = present(frame, assembled[TWK_PLANE_ALBEDO], assembled[TWK_PLANE_NORMAL], assembled[TWK_PLANE_MOMENTS], assembledGeometry);
    if (resolved) HIP_OK(hipFree(resolved));
    if (failed) return 1;
  }
  else if (cascadeEnabled)
  {
    // one device: resolve its own layers; the resolved picture is the frame. A denoiser takes it as an explicit beauty, so every
    // input it uses is passed beside it: copies of the handle's AOVs, and the handle's moments themselves
    TWK_OK(twk_cascade_resolve(devices[0], &cascade, &cascadeResolve, nullptr, 0, 0, nullptr));
    void* resolved = nullptr;
    TWK_OK(twk_get_resolved_device_pointer(devices[0], &resolved, nullptr));
    void* guides[2] = {nullptr, nullptr}; void* moments = nullptr;
    if (denoiserEnabled && denoiser.inputKind != TWK_DENOISER_RGB)
    {
      std::vector<unsigned char> host(numPixels * pixelBytes);
      HIP_OK(hipSetDevice(ordinals[0]));
      for (int which = 0; which < 2; ++which)
      {
        TWK_OK(twk_read_aov_raw(devices[0], which == 0 ? TWK_AOV_ALBEDO : TWK_AOV_NORMAL, host.data(), host.size()));
        HIP_OK(hipMalloc(&guides[which], host.size()));
        HIP_OK(hipMemcpy(guides[which], host.data(), host.size(), hipMemcpyHostToDevice));
      }
    }
    if (denoiserEnabled && denoiserSampledEnabled) TWK_OK(twk_get_moments_device_pointer(devices[0], &moments, nullptr));
    void* geometry = nullptr;
    if (geometryGuide)
    {
      TWK_OK(twk_render_geometry(devices[0]));
      TWK_OK(twk_get_geometry_device_pointer(devices[0], &geometry, nullptr));
    }
    const int failed = present(resolved, guides[0], guides[1], moments, geometry);
    for (void* guide : guides) if (guide) HIP_OK(hipFree(guide));
    if (failed) return 1;
  }
  else if (count == 1)
  {
    if (geometryGuide) TWK_OK(twk_render_geometry(devices[0])); // once, before the screenshot is filtered: the own-buffer form reads it
    if (present(nullptr)) return 1;
  }
  else if (sharedFrame)
  {
    // every device wrote its pixels straight into the frame
    if (present(sharedFrame)) return 1;
  }
  else
  {
    int launchWidth = 0;
    TWK_OK(twk_get_launch_width(devices[0], &launchWidth));
    const size_t tileBytes = (size_t) launchWidth * height * pixelBytes;
    void* tiles = nullptr; void* full = nullptr;
    HIP_OK(hipSetDevice(ordinals[0]));
    HIP_OK(hipMalloc(&tiles, tileBytes * count));
    HIP_OK(hipMalloc(&full, numPixels * pixelBytes));
    for (int i = 0; i < count; ++i)
    {
      void* src = nullptr; size_t bytes = 0;
      TWK_OK(twk_get_output_device_pointer(devices[(size_t) i], &src, &bytes));
      HIP_OK(hipMemcpyPeer(static_cast<char*>(tiles) + tileBytes * i, ordinals[0], src, ordinals[(size_t) i], tileBytes));
    }
    // device-to-device copies return before they have finished and the handle's stream is non-blocking: wait here,
    // or the compositor reads tiles that are still in flight
    HIP_OK(hipDeviceSynchronize());
    if (half) TWK_OK(twk_compositor_half(devices[0], tiles, full));
    else      TWK_OK(twk_compositor(devices[0], tiles, full));
    const int failed = present(full);
    HIP_OK(hipFree(tiles)); HIP_OK(hipFree(full));
    if (failed) return 1;
  }
  char path[4096];
  TWK_OK(twk_app_screenshot_path(app, 1, path, sizeof(path)));
  if (targetNoiseEnabled && iterationIndex != spp)
  {
    // the name carries the samples rendered: "<prefix>_<spp>spp_<date>..." with the count of this run
    std::string name(path);
    const std::string planned = "_" + std::to_string(spp) + "spp_", rendered = "_" + std::to_string(iterationIndex) + "spp_";
    const size_t at = name.rfind(planned);
    if (at != std::string::npos) name.replace(at, planned.size(), rendered);
    if (name.size() + 1 > sizeof(path)) { std::cerr << "ERROR: screenshot path too long\n"; return 1; }
    memcpy(path, name.c_str(), name.size() + 1);
  }
  TWK_OK(twk_write_png_rgb8(path, width, height, rgb8.data(), 1));
  std::cout << path << std::endl;

  for (int i = 0; i < count; ++i) TWK_OK(twk_device_destroy(devices[(size_t) i]));
  if (sharedFrame) { if (info.strategy == 1) (void) hipHostFree(sharedFrame); else (void) hipFree(sharedFrame); }
  TWK_OK(twk_app_destroy(app));
  return 0;
}

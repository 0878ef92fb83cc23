// The picture-shaped temporal merges behind the C ABI: the plain merge (temporal_device.h: the definition) and the rectified one
// (temporal_rectify_device.h). Their parameters and refusals, the explicit form, the own-buffer and the assembled form (temporalOwn
// serves both merges), the readers and the rectified merge's host-only form. The cascade's layers through the same reprojection are
// device_temporal_cascade.hip's, which takes its TwkTemporal checks and its history camera from here. The merged colour is a
// DevicePicture (device_handle.h); the history streams have its shape and are dropped and allocated with it.
#include "device_handle.h"
#include "temporal_motion_host.h"

#include <cstring>
#include <vector>

// Frees the streams of twk_temporal_accumulate's own-buffer form: the next call has no history
void twk::dropTemporal(TwkDevice dev)
{
  for (int s = 0; s < 2; ++s) for (int k = 0; k < 3; ++k) dev->d_temporal[s][k].release();
  dev->temporalColour.release();
  for (int s = 0; s < 2; ++s) dev->d_rectify[s].release();
  dev->d_temporalTrust.release();
  dev->temporalTrustValid = false; dev->temporalHasHistory = false;
  dev->d_temporalMotion.release(); dev->temporalMotion.clear(); dev->temporalTransforms.clear();
  dropPreviousPositions(dev, true);
  dropTemporalCascade(dev); // the merged layers of twk_temporal_enable_cascade are history of the same frames
}

// The two scratch streams of the rectified merge, at least `pixels` float4 each
static int ensureRectifyScratch(TwkDevice dev, size_t pixels)
{
  const int rc = growIdle(dev, dev->d_rectify[0], pixels);
  return rc ? rc : growIdle(dev, dev->d_rectify[1], pixels);
}

static TwkTemporal temporalDefaults()
{
  TwkTemporal tp; tp.maxHistory = TWK_TEMPORAL_MAX_HISTORY; tp.positionTolerance = TWK_TEMPORAL_POSITION_TOLERANCE;
  return tp;
}

static TwkTemporalRectify rectifyDefaults()
{
  TwkTemporalRectify rp; rp.radius = TWK_TEMPORAL_RECTIFY_RADIUS; rp.minTaps = TWK_TEMPORAL_RECTIFY_MIN_TAPS; rp.gamma = TWK_TEMPORAL_RECTIFY_GAMMA;
  return rp;
}

// The refusals of TwkTemporal's values (tp NULL: the defaults) and the constants they give: k zeroed but for maxHistory and tol2
int twk::temporalParameters(const char* name, const TwkTemporal* tp, TemporalConstants& k)
{
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  const TwkTemporal temporal = tp ? *tp : temporalDefaults();
  if (temporal.maxHistory < 1) return refuse("maxHistory must be >= 1");
  if (!(temporal.positionTolerance >= 0.0f) || !finite1(temporal.positionTolerance)) return refuse("positionTolerance must be >= 0 and finite");
  memset(&k, 0, sizeof(k));
  k.maxHistory = (float) temporal.maxHistory; k.tol2 = temporal.positionTolerance * temporal.positionTolerance;
  return TWK_SUCCESS;
}

// There is a history, rendered from `camera`: its part of the constants, or the refusal of a degenerate one
int twk::temporalHistoryCamera(const char* name, const TwkCameraDefinition& camera, TemporalConstants& k)
{
  k.hasHistory = 1;
  if (!temporalCamera(camera.P, k))
    return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": the history's camera is degenerate: U, V, W are linearly dependent or not finite");
  return TWK_SUCCESS;
}

// The refusals of the parameters every form of the rectified merge shares (tp, rp NULL: the defaults), and the constants they give;
// width, height unset
static int rectifyParameters(const char* name, const TwkTemporal* tp, const TwkTemporalRectify* rp, TemporalConstants& k, RectifyConstants& r)
{
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  const int rc = temporalParameters(name, tp, k); if (rc) return rc;
  const TwkTemporalRectify rectify = rp ? *rp : rectifyDefaults();
  static_assert(TWK_TEMPORAL_RECTIFY_MAX_RADIUS == TWK_RECTIFY_MAX_RADIUS, "the header's largest radius is the kernel's");
  if (rectify.radius < 1 || rectify.radius > TWK_RECTIFY_MAX_RADIUS) return refuse("radius must be in 1..4");
  if (rectify.minTaps < 2) return refuse("minTaps must be >= 2 (a variance needs two taps)");
  if (!(rectify.gamma >= 0.0f) || !finite1(rectify.gamma)) return refuse("gamma must be >= 0 and finite");
  r.radius = rectify.radius; r.minTaps = rectify.minTaps; r.gamma2 = rectify.gamma * rectify.gamma;
  return TWK_SUCCESS;
}

// The table of the own-buffer merge about to be issued: one record per instance when the history's snapshot of the transforms
// differs from the transforms as they are, uploaded on the stream; none (temporalMotion empty) while no instance has moved —
// the only state there is without twk_update_instance_transform — or without a history.
static int ownMotion(TwkDevice dev, const char* name)
{
  dev->temporalMotion.clear();
  const size_t count = dev->instances.size();
  if (!dev->temporalHasHistory || dev->temporalTransforms.size() != 12 * count) return TWK_SUCCESS;
  bool moved = false;
  for (size_t i = 0; i < count && !moved; ++i) moved = memcmp(&dev->temporalTransforms[12 * i], dev->instances[i].transform, 12 * sizeof(float)) != 0;
  if (!moved) return TWK_SUCCESS;
  std::vector<TwkInstanceMotion> table(count);
  for (size_t i = 0; i < count; ++i)
  {
    const float* previous = &dev->temporalTransforms[12 * i];
    const float* current = dev->instances[i].transform;
    memset(&table[i], 0, sizeof(TwkInstanceMotion));
    if (memcmp(previous, current, 12 * sizeof(float)) == 0) { table[i].previousFromCurrent[0] = table[i].previousFromCurrent[5] = table[i].previousFromCurrent[10] = 1.0f; continue; }
    if (!instanceMotion(previous, current, table[i]))
      return twkSetError(TWK_ERROR_INVALID_STATE, std::string(name) + ": instance " + std::to_string(i) + " has moved and its transform, now or in the history's frame, is singular or not finite");
  }
  const int rc = growIdle(dev, dev->d_temporalMotion, count); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(dev->d_temporalMotion, table.data(), count * sizeof(TwkInstanceMotion), hipMemcpyHostToDevice, dev->stream));
  HIP_TRY(hipStreamSynchronize(dev->stream)); // (the table is pageable host memory that goes out of use here; a move is rare and has just rebuilt the scene)
  dev->temporalMotion.swap(table);
  return TWK_SUCCESS;
}

// The merge of the own-buffer form and of the assembled form, after their refusals: the frame (colour in the output format,
// moments, geometry; layers: the cascade layers to merge while twk_temporal_enable_cascade is on, nullptr = the handle's own) of
// width x height pixels against the history the handle kept, which it then replaces — looked up where each instance was when
// twk_update_instance_transform has moved one since (ownMotion). k: maxHistory and tol2 are set. rectify:
// nullptr = the plain merge; else the rectified one (temporal_rectify_device.h), which also writes the handle's trust plane and,
// while twk_temporal_enable_cascade is on, discounts the layers' history by it.
static int temporalOwn(TwkDevice dev, const char* name, TemporalConstants k, const RectifyConstants* rectify, const void* colour, const float4* moments, const float4* geometry,
                       const float4* layers, int width, int height)
{
  const size_t n = (size_t) width * height;
  int rc;
  if (!dev->temporalColour.shaped(width, height, dev->outputFormat))
  {
    // the history has the picture's shape and goes with it: dropped (once everything enqueued has run), then allocated with it
    HIP_TRY(hipStreamSynchronize(dev->stream));
    dropTemporal(dev);
    for (int s = 0; s < 2; ++s) for (int j = 0; j < 3; ++j) if ((rc = dev->d_temporal[s][j].allocate(n))) return rc;
    if ((rc = ensurePicture(dev, dev->temporalColour, width, height))) return rc;
    dev->temporalKept = 0;
  }
  const float4 *hColour = nullptr, *hMoments = nullptr, *hGeometry = nullptr;
  if (dev->temporalHasHistory)
  {
    const DeviceArray<float4>* h = dev->d_temporal[dev->temporalKept];
    hColour = h[0]; hMoments = h[1]; hGeometry = h[2];
  }
  const int keep = dev->temporalHasHistory ? 1 - dev->temporalKept : dev->temporalKept;
  k.width = width; k.height = height;
  if (dev->temporalHasHistory && (rc = temporalHistoryCamera(name, dev->temporalCamera, k))) return rc;
  // while a geometry is deformed the Carried builds run: g' from the previous-position plane (temporal_carry_device.h), which holds
  // X g of a moved instance already, so no table is built; the callers have refused a deformed geometry without a valid plane
  const float4* carried = (dev->temporalHasHistory && geometryDeformed(dev)) ? dev->d_previousPlane.get() : nullptr;
  if (carried) dev->temporalMotion.clear();
  else if ((rc = ownMotion(dev, name))) return rc;
  const TwkInstanceMotion* motion = dev->temporalMotion.empty() ? nullptr : dev->d_temporalMotion.get();
  const unsigned int numMotion = (unsigned int) dev->temporalMotion.size();
  // twk_temporal_enable_cascade: the layers through the same previous geometry and camera, before the history is swapped
  if (rectify)
  {
    // the trust first: the layers' merge reads it
    if ((rc = ensureRectifyScratch(dev, n))) return rc;
    if ((rc = dev->d_temporalTrust.ensure(n))) return rc;
    launchTemporalRectify(colour, halfOutput(dev), moments, geometry, hColour, hMoments, hGeometry, dev->d_rectify[0], dev->d_rectify[1], dev->temporalColour.pixels,
                          dev->d_temporal[keep][0], dev->d_temporal[keep][1], dev->d_temporalTrust, k, *rectify, dev->stream, motion, numMotion, carried);
    HIP_TRY(hipGetLastError());
    if (dev->temporalCascade && (rc = temporalCascadeOwn(dev, k, layers, geometry, hGeometry, dev->d_temporalTrust, motion, numMotion, carried))) return rc;
    dev->temporalTrustValid = true;
  }
  else
  {
    if (dev->temporalCascade && (rc = temporalCascadeOwn(dev, k, layers, geometry, hGeometry, nullptr, motion, numMotion, carried))) return rc;
    launchTemporal(colour, halfOutput(dev), moments, geometry, hColour, hMoments, hGeometry, dev->temporalColour.pixels, dev->d_temporal[keep][0], dev->d_temporal[keep][1], k, dev->stream,
                   motion, numMotion, carried);
    HIP_TRY(hipGetLastError());
    dev->temporalTrustValid = false; // the trust plane, if any, is an earlier frame's
  }
  HIP_TRY(hipMemcpyAsync(dev->d_temporal[keep][2], geometry, n * sizeof(float4), hipMemcpyDeviceToDevice, dev->stream));
  dev->temporalKept = keep; dev->temporalCamera = dev->cameras[0]; dev->temporalHasHistory = true; dev->temporalColour.valid = true;
  dev->temporalTransforms.resize(12 * dev->instances.size()); // the history now is this frame: its instances are where they are
  for (size_t i = 0; i < dev->instances.size(); ++i) memcpy(&dev->temporalTransforms[12 * i], dev->instances[i].transform, 12 * sizeof(float));
  dropPreviousPositions(dev, false); // ... and its vertices are where they are: no geometry is deformed, the plane describes the history that was
  return TWK_SUCCESS;
}

// The own-buffer form of twk_temporal_accumulate and of twk_temporal_accumulate_rectified after the checks of their arguments: the
// refusals of the handle's state, then the merge. k: maxHistory and tol2 are set.
static int temporalOwnFrame(TwkDevice dev, const char* name, const TemporalConstants& k, const RectifyConstants* rectify)
{
  const auto refuse = [name](int code, const char* text) { return twkSetError(code, (std::string(name) + ": " + text).c_str()); };
  if (!dev->stateSet || dev->cameras.empty()) return refuse(TWK_ERROR_INVALID_STATE, "twk_set_state and twk_init_cameras first");
  if (dev->state.distribution && 1 < dev->count) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffer is a packed tile buffer (distribution 1, more than one device), not a picture");
  const int width = dev->launchWidth, height = dev->state.resolution[1];
  const size_t n = (size_t) width * height;
  if (!ownMoments(dev, n)) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffers have no luminance moments: render with twk_enable_moments(1)");
  if (!ownGeometry(dev, n)) return refuse(TWK_ERROR_INVALID_STATE, "the handle's own buffers have no geometry AOV: twk_enable_geometry(1) and twk_render_geometry");
  if (!dev->geometryValid) return refuse(TWK_ERROR_INVALID_STATE, "the geometry AOV is older than the camera, the state or the scene: twk_render_geometry first");
  const void* colour = ownOutput(dev, n);
  if (!colour) return refuse(TWK_ERROR_INVALID_STATE, "nothing has been rendered");
  if (dev->temporalCascade) if (const char* why = temporalCascadeRefusal(dev)) return refuse(TWK_ERROR_INVALID_STATE, why);
  if (dev->temporalHasHistory && geometryDeformed(dev) && !(dev->previousPlaneValid && dev->d_previousPlane.holds(n)))
    return refuse(TWK_ERROR_INVALID_STATE, "a geometry is deformed (twk_update_geometry_vertices since the history's frame) and there is no valid previous-position plane: twk_render_geometry_motion first");
  return temporalOwn(dev, name, k, rectify, colour, dev->d_moments, dev->d_geometry, nullptr, width, height);
}

// twk_temporal_accumulate_assembled and twk_temporal_accumulate_assembled_rectified after the checks of their parameters
static int temporalAssembledFrame(TwkDevice dev, const char* name, const TemporalConstants& k, const RectifyConstants* rectify)
{
  const auto refuse = [name](int code, const std::string& text) { return twkSetError(code, std::string(name) + ": " + text); };
  if (!dev->stateSet || dev->cameras.empty()) return refuse(TWK_ERROR_INVALID_STATE, "twk_set_state and twk_init_cameras first");
  if (!(dev->state.distribution && 1 < dev->count))
    return refuse(TWK_ERROR_INVALID_STATE, "the handle is not tiled (distribution 1, more than one device): its own buffers are the picture, twk_temporal_accumulate merges them");
  if (geometryDeformed(dev)) return refuse(TWK_ERROR_INVALID_STATE, "a geometry is deformed (twk_update_geometry_vertices since the history's frame): the previous-position plane is not built on tiled frames; twk_temporal_reset first");
  if (!dev->momentsEnabled) return refuse(TWK_ERROR_INVALID_STATE, "the frame has no luminance moments: render with twk_enable_moments(1)");
  if (!dev->geometryEnabled) return refuse(TWK_ERROR_INVALID_STATE, "the frame has no geometry AOV: twk_enable_geometry(1) and twk_render_geometry_tile");
  if (dev->temporalCascade) if (const char* why = temporalCascadeRefusal(dev)) return refuse(TWK_ERROR_INVALID_STATE, why);
  const int needed[3] = {TWK_PLANE_OUTPUT, TWK_PLANE_MOMENTS, TWK_PLANE_CASCADE};
  static const char* const neededNames[3] = {"TWK_PLANE_OUTPUT", "TWK_PLANE_MOMENTS", "TWK_PLANE_CASCADE"};
  for (int j = 0; j < (dev->temporalCascade ? 3 : 2); ++j)
    if (!dev->assembledValid[needed[j]] || !dev->d_assembled[needed[j]])
      return refuse(TWK_ERROR_INVALID_STATE, std::string(neededNames[j]) + " has not been assembled on this handle: twk_assemble_devices_with_geometry first");
  if (!dev->d_assembledGeometry) return refuse(TWK_ERROR_INVALID_STATE, "the geometry AOV has not been assembled on this handle: twk_assemble_devices_with_geometry first");
  if (!dev->assembledGeometryValid) return refuse(TWK_ERROR_INVALID_STATE, "the assembled geometry AOV is stale, older than the camera, the state or the scene: twk_render_geometry_tile and twk_assemble_devices_with_geometry first");
  return temporalOwn(dev, name, k, rectify, dev->d_assembled[TWK_PLANE_OUTPUT], static_cast<const float4*>(dev->d_assembled[TWK_PLANE_MOMENTS].get()), static_cast<const float4*>(dev->d_assembledGeometry.get()),
                     dev->temporalCascade ? static_cast<const float4*>(dev->d_assembled[TWK_PLANE_CASCADE].get()) : nullptr, dev->state.resolution[0], dev->state.resolution[1]);
}

// twk_temporal_accumulate (rectify nullptr, no trustOut) and twk_temporal_accumulate_rectified after the checks of their parameters,
// on an active handle: without a current frame the own-buffer form, else the explicit form's refusals and its launch. motion,
// numMotion: the table of twk_temporal_accumulate_moving (a device pointer; nullptr or 0: none, the launches of the other two).
static int temporalFrame(TwkDevice dev, const char* name, TemporalConstants k, const RectifyConstants* rectify, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                         int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut, const TwkInstanceMotion* motion = nullptr, int numMotion = 0,
                         const void* previousPositions = nullptr)
{
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!current)
  {
    if (history || colourOut || historyOut || momentsOut || trustOut || width || height)
      return refuse("a history, outputs or a size without a current frame (pass both frames, or neither for the handle's own buffers)");
    return temporalOwnFrame(dev, name, k, rectify);
  }
  if (width < 1 || height < 1 || (size_t) width * (size_t) height >= ((size_t) 1 << 31)) return refuse("width and height must be >= 1");
  if (!current->colour || !current->moments || !current->geometry) return refuse("NULL buffer in the current frame");
  if (history && (!history->colour || !history->moments || !history->geometry)) return refuse("NULL buffer in the history frame");
  const void* colour = current->colour;
  const float4 *moments = static_cast<const float4*>(current->moments), *geometry = static_cast<const float4*>(current->geometry);
  const float4 *hColour = nullptr, *hMoments = nullptr, *hGeometry = nullptr;
  if (history) { hColour = static_cast<const float4*>(history->colour); hMoments = static_cast<const float4*>(history->moments); hGeometry = static_cast<const float4*>(history->geometry); }
  const size_t n = (size_t) width * height, wide = n * sizeof(float4), narrowBytes = n * pixelBytes(dev);
  const void* outs[4] = {colourOut, historyOut, momentsOut, trustOut}; const size_t outBytes[4] = {narrowBytes, wide, wide, n * sizeof(float)};
  const void* ins[6] = {colour, moments, geometry, hColour, hMoments, hGeometry}; const size_t inBytes[6] = {narrowBytes, wide, wide, wide, wide, wide};
  for (int o = 0; o < 4; ++o)
  {
    for (int i = 0; i < 6; ++i) if (overlaps(outs[o], outBytes[o], ins[i], inBytes[i])) return refuse("an output overlaps an input (the kernel gathers the history at other pixels)");
    for (int j = o + 1; j < 4; ++j) if (overlaps(outs[o], outBytes[o], outs[j], outBytes[j])) return refuse("two outputs overlap");
  }
  if (!motion || !history) numMotion = 0; // (without a history nothing is reprojected)
  if (numMotion > 0 && ((uintptr_t) motion & 15u) != 0) return refuse("the motion table is not 16-byte aligned");
  for (int o = 0; o < 4 && numMotion > 0; ++o)
    if (overlaps(outs[o], outBytes[o], motion, (size_t) numMotion * sizeof(TwkInstanceMotion))) return refuse("an output overlaps the motion table");
  // the previous-position plane of a Carried build (twk_temporal_accumulate_carried); without a history nothing is reprojected
  const float4* carried = history ? static_cast<const float4*>(previousPositions) : nullptr;
  if (carried && ((uintptr_t) carried & 15u) != 0) return refuse("the previous positions are not 16-byte aligned");
  for (int o = 0; o < 4 && carried; ++o) if (overlaps(outs[o], outBytes[o], carried, wide)) return refuse("an output overlaps the previous positions");
  k.width = width; k.height = height;
  int rc;
  if (history && (rc = temporalHistoryCamera(name, history->camera, k))) return rc;
  if (rectify)
  {
    if ((rc = ensureRectifyScratch(dev, n))) return rc;
    launchTemporalRectify(colour, halfOutput(dev), moments, geometry, hColour, hMoments, hGeometry, dev->d_rectify[0], dev->d_rectify[1], colourOut, static_cast<float4*>(historyOut),
                          static_cast<float4*>(momentsOut), static_cast<float*>(trustOut), k, *rectify, dev->stream, motion, (unsigned int) numMotion, carried);
  }
  else
    launchTemporal(colour, halfOutput(dev), moments, geometry, hColour, hMoments, hGeometry, colourOut, static_cast<float4*>(historyOut), static_cast<float4*>(momentsOut), k, dev->stream,
                   motion, (unsigned int) numMotion, carried);
  HIP_TRY(hipGetLastError());
  return TWK_SUCCESS;
}

// The readers' refusal while the handle holds no own-buffer result
static const char* const noTemporal = "no twk_temporal_accumulate on the handle's own buffers since the last reset";
static const char* const noTrust = "the last merge on the handle's own buffers was no twk_temporal_accumulate_rectified, or its history has been dropped";

extern "C" {

int twk_temporal_defaults(TwkTemporal* tp)
try
{
  if (!tp) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_temporal_defaults: NULL argument");
  *tp = temporalDefaults();
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_defaults")

int twk_temporal_rectify_defaults(TwkTemporalRectify* rp)
try
{
  if (!rp) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_temporal_rectify_defaults: NULL argument");
  *rp = rectifyDefaults();
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_rectify_defaults")

int twk_temporal_accumulate(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalFrame* current, const TwkTemporalFrame* history, int width, int height,
                            void* colourOut, void* historyOut, void* momentsOut)
try
{
  const char* name = "twk_temporal_accumulate";
  int rc = activate(dev, name); if (rc) return rc;
  TemporalConstants k;
  if ((rc = temporalParameters(name, tp, k))) return rc;
  return temporalFrame(dev, name, k, nullptr, current, history, width, height, colourOut, historyOut, momentsOut, nullptr);
}
TWK_CATCH("twk_temporal_accumulate")

int twk_temporal_accumulate_rectified(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalRectify* rp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                                      int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut)
try
{
  const char* name = "twk_temporal_accumulate_rectified";
  int rc = activate(dev, name); if (rc) return rc;
  TemporalConstants k;
  RectifyConstants r;
  if ((rc = rectifyParameters(name, tp, rp, k, r))) return rc;
  return temporalFrame(dev, name, k, &r, current, history, width, height, colourOut, historyOut, momentsOut, trustOut);
}
TWK_CATCH("twk_temporal_accumulate_rectified")

int twk_temporal_accumulate_moving(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalRectify* rp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                                   const TwkInstanceMotion* motion, int numMotion, int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut)
try
{
  const char* name = "twk_temporal_accumulate_moving";
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  int rc = activate(dev, name); if (rc) return rc;
  TemporalConstants k;
  RectifyConstants r;
  if ((rc = rp ? rectifyParameters(name, tp, rp, k, r) : temporalParameters(name, tp, k))) return rc;
  if (!current) return refuse("NULL current frame (the explicit form only: twk_temporal_accumulate's own-buffer form builds its table itself)");
  if (!rp && trustOut) return refuse("a trustOut without TwkTemporalRectify (rp NULL is the plain merge)");
  if (numMotion < 0) return refuse("numMotion must be >= 0");
  return temporalFrame(dev, name, k, rp ? &r : nullptr, current, history, width, height, colourOut, historyOut, momentsOut, trustOut, motion, numMotion);
}
TWK_CATCH("twk_temporal_accumulate_moving")

int twk_temporal_accumulate_carried(TwkDevice dev, const TwkTemporal* tp, const TwkTemporalRectify* rp, const TwkTemporalFrame* current, const TwkTemporalFrame* history,
                                    const void* previousPositions, int width, int height, void* colourOut, void* historyOut, void* momentsOut, void* trustOut)
try
{
  const char* name = "twk_temporal_accumulate_carried";
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  int rc = activate(dev, name); if (rc) return rc;
  TemporalConstants k;
  RectifyConstants r;
  if ((rc = rp ? rectifyParameters(name, tp, rp, k, r) : temporalParameters(name, tp, k))) return rc;
  if (!current) return refuse("NULL current frame (the explicit form only: twk_temporal_accumulate's own-buffer form reads the handle's plane itself)");
  if (!rp && trustOut) return refuse("a trustOut without TwkTemporalRectify (rp NULL is the plain merge)");
  return temporalFrame(dev, name, k, rp ? &r : nullptr, current, history, width, height, colourOut, historyOut, momentsOut, trustOut, nullptr, 0, previousPositions);
}
TWK_CATCH("twk_temporal_accumulate_carried")

int twk_read_temporal_motion(TwkDevice dev, TwkInstanceMotion* host, size_t capacity, int* count)
try
{
  const char* name = "twk_read_temporal_motion";
  if (!dev || !count) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + (dev ? ": NULL count" : ": NULL device handle"));
  const size_t used = dev->temporalMotion.size();
  *count = (int) used; // (written before the capacity is held against it: a call with capacity 0 asks for the count)
  if (capacity < used || (used > 0 && !host)) return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": the table has " + std::to_string(used) + " records, more than the capacity given");
  if (used > 0) memcpy(host, dev->temporalMotion.data(), used * sizeof(TwkInstanceMotion));
  return TWK_SUCCESS;
}
TWK_CATCH("twk_read_temporal_motion")

int twk_instance_motion(const float previous[12], const float current[12], TwkInstanceMotion* out)
try
{
  if (!previous || !current || !out) return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_instance_motion: NULL argument");
  if (!instanceMotion(previous, current, *out))
    return twkSetError(TWK_ERROR_INVALID_VALUE, "twk_instance_motion: an input is not finite, or the 3 x 3 determinant of current is zero or not finite");
  return TWK_SUCCESS;
}
TWK_CATCH("twk_instance_motion")

int twk_temporal_accumulate_assembled(TwkDevice primary, const TwkTemporal* tp)
try
{
  const char* name = "twk_temporal_accumulate_assembled";
  int rc = activate(primary, name); if (rc) return rc;
  TemporalConstants k;
  if ((rc = temporalParameters(name, tp, k))) return rc;
  return temporalAssembledFrame(primary, name, k, nullptr);
}
TWK_CATCH("twk_temporal_accumulate_assembled")

int twk_temporal_accumulate_assembled_rectified(TwkDevice primary, const TwkTemporal* tp, const TwkTemporalRectify* rp)
try
{
  const char* name = "twk_temporal_accumulate_assembled_rectified";
  int rc = activate(primary, name); if (rc) return rc;
  TemporalConstants k;
  RectifyConstants r;
  if ((rc = rectifyParameters(name, tp, rp, k, r))) return rc;
  return temporalAssembledFrame(primary, name, k, &r);
}
TWK_CATCH("twk_temporal_accumulate_assembled_rectified")

int twk_temporal_reset(TwkDevice dev)
try
{
  int rc = activate(dev, "twk_temporal_reset"); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dropTemporal(dev);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_reset")

int twk_get_temporal_device_pointers(TwkDevice dev, void** colour, size_t* colourBytes, void** moments, size_t* momentsBytes)
try
{
  const std::string name = "twk_get_temporal_device_pointers";
  int rc = activate(dev, name.c_str()); if (rc) return rc;
  const DevicePicture& picture = dev->temporalColour;
  if (!picture.valid) return twkSetError(TWK_ERROR_INVALID_STATE, name + ": " + noTemporal);
  if (colour) *colour = picture.pixels;
  if (colourBytes) *colourBytes = picture.count() * pixelBytes(picture.format);
  if (moments) *moments = dev->d_temporal[dev->temporalKept][1];
  if (momentsBytes) *momentsBytes = picture.count() * sizeof(float4);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_get_temporal_device_pointers")

int twk_read_temporal(TwkDevice dev, float* rgbaHost, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_temporal"); if (rc) return rc;
  return readBack(dev, "twk_read_temporal", {currentPicture(dev, dev->temporalColour), noTemporal, dev->temporalColour.count(), 0, true}, rgbaHost, numFloats, 4, "width*height*4 floats");
}
TWK_CATCH("twk_read_temporal")

int twk_read_temporal_moments(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_temporal_moments"); if (rc) return rc;
  const float4* kept = dev->temporalColour.valid ? dev->d_temporal[dev->temporalKept][1].get() : nullptr;
  return readBack(dev, "twk_read_temporal_moments", {kept, noTemporal, dev->temporalColour.count(), sizeof(float4), true}, host, numFloats, 4, "width*height*4 floats");
}
TWK_CATCH("twk_read_temporal_moments")

// The trust plane of the last own-buffer merge, if that was a rectified one
static float* ownTrust(TwkDevice dev) { return (dev->temporalColour.valid && dev->temporalTrustValid) ? dev->d_temporalTrust.get() : nullptr; }

int twk_get_temporal_trust_device_pointer(TwkDevice dev, void** dptr, size_t* bytes)
try
{
  return getPointer(dev, "twk_get_temporal_trust_device_pointer", dptr, bytes, [dev](void*& pointer, size_t& size)
  {
    if (!(pointer = ownTrust(dev))) return twkSetError(TWK_ERROR_INVALID_STATE, std::string("twk_get_temporal_trust_device_pointer: ") + noTrust);
    size = dev->temporalColour.count() * sizeof(float);
    return (int) TWK_SUCCESS;
  });
}
TWK_CATCH("twk_get_temporal_trust_device_pointer")

int twk_read_temporal_trust(TwkDevice dev, float* host, size_t numFloats)
try
{
  int rc = activate(dev, "twk_read_temporal_trust"); if (rc) return rc;
  return readBack(dev, "twk_read_temporal_trust", {ownTrust(dev), noTrust, dev->temporalColour.count(), sizeof(float), true}, host, numFloats, 1, "width*height floats");
}
TWK_CATCH("twk_read_temporal_trust")

int twk_temporal_rectify_host(const TwkTemporal* tp, const TwkTemporalRectify* rp, const float* colour, const float* moments, const float* geometry,
                              const float* historyColour, const float* historyMoments, const float* historyGeometry, const TwkCameraDefinition* historyCamera,
                              int width, int height, float* colourOut, float* momentsOut, float* trustOut)
try
{
  const char* name = "twk_temporal_rectify_host";
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!colour || !moments || !geometry) return refuse("NULL buffer in the current frame");
  const bool history = historyColour || historyMoments || historyGeometry;
  if (history && (!historyColour || !historyMoments || !historyGeometry || !historyCamera)) return refuse("a history without its colour, moments, geometry or camera");
  TemporalConstants k;
  RectifyConstants r;
  int rc = rectifyParameters(name, tp, rp, k, r); if (rc) return rc;
  if (width < 1 || height < 1 || (size_t) width * (size_t) height > ((size_t) 1 << 28)) return refuse("width and height must be >= 1, width*height at most 2^28");
  k.width = width; k.height = height;
  if (history && (rc = temporalHistoryCamera(name, *historyCamera, k))) return rc;
  const TemporalHostFrame frame((size_t) width * height, colour, moments, geometry, historyColour, historyMoments, historyGeometry);
  temporalRectifyHost<false>(k, r, frame, nullptr, 0u, colourOut, momentsOut, trustOut);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_rectify_host")

int twk_temporal_moving_host(const TwkTemporal* tp, const TwkTemporalRectify* rp, const float* colour, const float* moments, const float* geometry,
                             const float* historyColour, const float* historyMoments, const float* historyGeometry, const TwkCameraDefinition* historyCamera,
                             const TwkInstanceMotion* motion, int numMotion, int width, int height, float* colourOut, float* momentsOut, float* trustOut)
try
{
  const char* name = "twk_temporal_moving_host";
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!colour || !moments || !geometry) return refuse("NULL buffer in the current frame");
  const bool history = historyColour || historyMoments || historyGeometry;
  if (history && (!historyColour || !historyMoments || !historyGeometry || !historyCamera)) return refuse("a history without its colour, moments, geometry or camera");
  if (!rp && trustOut) return refuse("a trustOut without TwkTemporalRectify (rp NULL is the plain merge)");
  if (numMotion < 0) return refuse("numMotion must be >= 0");
  TemporalConstants k;
  RectifyConstants r;
  int rc = rp ? rectifyParameters(name, tp, rp, k, r) : temporalParameters(name, tp, k); if (rc) return rc;
  if (width < 1 || height < 1 || (size_t) width * (size_t) height > ((size_t) 1 << 28)) return refuse("width and height must be >= 1, width*height at most 2^28");
  k.width = width; k.height = height;
  if (history && (rc = temporalHistoryCamera(name, *historyCamera, k))) return rc;
  const TemporalHostFrame frame((size_t) width * height, colour, moments, geometry, historyColour, historyMoments, historyGeometry);
  temporalMergeHost(k, rp ? &r : nullptr, frame, motion, motion ? (unsigned int) numMotion : 0u, colourOut, momentsOut, trustOut);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_moving_host")

int twk_temporal_carried_host(const TwkTemporal* tp, const TwkTemporalRectify* rp, const float* colour, const float* moments, const float* geometry,
                              const float* historyColour, const float* historyMoments, const float* historyGeometry, const TwkCameraDefinition* historyCamera,
                              const float* previousPositions, int width, int height, float* colourOut, float* momentsOut, float* trustOut)
try
{
  const char* name = "twk_temporal_carried_host";
  const auto refuse = [name](const char* text) { return twkSetError(TWK_ERROR_INVALID_VALUE, std::string(name) + ": " + text); };
  if (!colour || !moments || !geometry) return refuse("NULL buffer in the current frame");
  const bool history = historyColour || historyMoments || historyGeometry;
  if (history && (!historyColour || !historyMoments || !historyGeometry || !historyCamera)) return refuse("a history without its colour, moments, geometry or camera");
  if (!rp && trustOut) return refuse("a trustOut without TwkTemporalRectify (rp NULL is the plain merge)");
  TemporalConstants k;
  RectifyConstants r;
  int rc = rp ? rectifyParameters(name, tp, rp, k, r) : temporalParameters(name, tp, k); if (rc) return rc;
  if (width < 1 || height < 1 || (size_t) width * (size_t) height > ((size_t) 1 << 28)) return refuse("width and height must be >= 1, width*height at most 2^28");
  k.width = width; k.height = height;
  if (history && (rc = temporalHistoryCamera(name, *historyCamera, k))) return rc;
  const TemporalHostFrame frame((size_t) width * height, colour, moments, geometry, historyColour, historyMoments, historyGeometry);
  temporalMergeHost(k, rp ? &r : nullptr, frame, nullptr, 0u, colourOut, momentsOut, trustOut, history ? previousPositions : nullptr);
  return TWK_SUCCESS;
}
TWK_CATCH("twk_temporal_carried_host")

} // extern "C"

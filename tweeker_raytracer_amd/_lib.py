"""ctypes loader of libtweeker_hip.so — the C ABI declared in include/tweeker_hip.h.

There is no Python or CPU fallback: if the HIP library is missing the import fails loudly, and every
compute entry point fails with TWK_ERROR_NO_DEVICE on a machine without a GPU.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TWK_LIB") or os.path.join(_HERE, "libtweeker_hip.so")  # TWK_LIB: an A/B variant built by tools/ab_variant.sh


class TwkError(RuntimeError):
    """≙ the std::runtime_error thrown by CU_CHECK/OPTIX_CHECK (reference inc/CheckMacros.h:38-80)."""

    def __init__(self, code, message):
        super().__init__(f"tweeker_hip error {code}: {message}")
        self.code = code


TWK_SUCCESS, TWK_ERROR_INVALID_VALUE, TWK_ERROR_NO_DEVICE, TWK_ERROR_HIP = 0, 1, 2, 3
TWK_ERROR_INVALID_STATE, TWK_ERROR_OUT_OF_MEMORY, TWK_ERROR_IO, TWK_ERROR_PARSE = 4, 5, 6, 7
TWK_OUTPUT_FLOAT4, TWK_OUTPUT_HALF4 = 0, 1  # twk_set_output_format: RGBA32F (default), RGBA16F (≙ Optix7Gui USE_FP32_OUTPUT 0)

TWK_DENOISER_RGB, TWK_DENOISER_RGB_ALBEDO, TWK_DENOISER_RGB_ALBEDO_NORMAL = 0, 1, 2  # TwkDenoiser.inputKind: the guides that weigh the taps
TWK_DENOISER_SIGMA_POSITION = 0.01  # twk_denoiser_geometry_defaults (include/tweeker_hip.h)
TWK_DENOISER_MIN_SAMPLES = 4  # default "denoiserMinSamples" of twk_denoise_variance_sampled (include/tweeker_hip.h)

TWK_TEMPORAL_MAX_HISTORY, TWK_TEMPORAL_POSITION_TOLERANCE = 32, 0.01  # twk_temporal_defaults (include/tweeker_hip.h)
TWK_TEMPORAL_RECTIFY_RADIUS, TWK_TEMPORAL_RECTIFY_MIN_TAPS, TWK_TEMPORAL_RECTIFY_GAMMA, TWK_TEMPORAL_RECTIFY_MAX_RADIUS = 3, 8, 3.0, 4  # twk_temporal_rectify_defaults (provisional)
TWK_NOISE_DARK_FLOOR = 0.01  # twk_noise_defaults (include/tweeker_hip.h); its minSamples is TWK_DENOISER_MIN_SAMPLES
TWK_ADAPTIVE_TARGET_NOISE, TWK_ADAPTIVE_MAX_SAMPLES = 0.05, 4096  # twk_adaptive_defaults (include/tweeker_hip.h)
TWK_CASCADE_LAYERS, TWK_CASCADE_START, TWK_CASCADE_BASE = 6, 1.0, 8.0  # twk_cascade_defaults (include/tweeker_hip.h)
TWK_CASCADE_KAPPA = 32.0  # twk_cascade_resolve_defaults (provisional: profiles/r15_cascade.md)
# twk_assemble: the planes of a tiled frame (include/tweeker_hip.h "Assembling a tiled frame"); a plane mask is 1 << plane ored together
TWK_PLANE_OUTPUT, TWK_PLANE_ALBEDO, TWK_PLANE_NORMAL, TWK_PLANE_MOMENTS, TWK_PLANE_SAMPLE_COUNTS, TWK_PLANE_CASCADE = 0, 1, 2, 3, 4, 5
TWK_PLANE_COUNT = 6

f3 = C.c_float * 3
f2 = C.c_float * 2
i2 = C.c_int * 2


class CameraDefinition(C.Structure):
    _fields_ = [("P", f3), ("U", f3), ("V", f3), ("W", f3)]


class LightDefinition(C.Structure):
    _fields_ = [("type", C.c_int), ("position", f3), ("vecU", f3), ("vecV", f3), ("normal", f3),
                ("area", C.c_float), ("emission", f3), ("unused0", C.c_float), ("unused1", C.c_float),
                ("unused2", C.c_float)]


class MaterialGUI(C.Structure):
    _fields_ = [("indexBSDF", C.c_int), ("albedo", f3), ("absorptionColor", f3), ("absorptionScale", C.c_float),
                ("ior", C.c_float), ("thinwalled", C.c_int), ("useAlbedoTexture", C.c_int),
                ("useCutoutTexture", C.c_int), ("roughness", f2)]


class TriangleAttributes(C.Structure):
    _fields_ = [("vertex", f3), ("tangent", f3), ("normal", f3), ("texcoord", f3)]


class DeviceState(C.Structure):
    _fields_ = [("resolution", i2), ("tileSize", i2), ("pathLengths", i2), ("distribution", C.c_int),
                ("samplesSqrt", C.c_int), ("lensShader", C.c_int), ("epsilonFactor", C.c_float),
                ("envRotation", C.c_float), ("clockFactor", C.c_float)]


class Tonemapper(C.Structure):
    """≙ TonemapperGUI (inc/TonemapperGUI.h:34-43); neutral defaults of Application.cpp:111-120."""
    _fields_ = [("gamma", C.c_float), ("whitePoint", C.c_float), ("colorBalance", C.c_float * 3),
                ("burnHighlights", C.c_float), ("crushBlacks", C.c_float), ("saturation", C.c_float),
                ("brightness", C.c_float)]

    def __init__(self, gamma=1.0, whitePoint=1.0, colorBalance=(1.0, 1.0, 1.0), burnHighlights=1.0, crushBlacks=0.0,
                 saturation=1.0, brightness=1.0):
        super().__init__(gamma, whitePoint, (C.c_float * 3)(*colorBalance), burnHighlights, crushBlacks, saturation, brightness)


class Denoiser(C.Structure):
    """≙ TwkDenoiser: parameters of twk_denoise, the edge-avoiding a-trous wavelet filter at the optixDenoiserInvoke seam
    (inputKind + blendFactor ≙ OptixDenoiserOptions / OptixDenoiserParams). Without arguments: twk_denoiser_defaults."""
    _fields_ = [("inputKind", C.c_int), ("iterations", C.c_int), ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float),
                ("sigmaAlbedo", C.c_float), ("demodulateAlbedo", C.c_int), ("blendFactor", C.c_float)]

    def __init__(self, inputKind=TWK_DENOISER_RGB_ALBEDO_NORMAL, iterations=3, sigmaColor=8.0, sigmaNormal=0.3, sigmaAlbedo=0.1,
                 demodulateAlbedo=None, blendFactor=0.0):
        if demodulateAlbedo is None:
            demodulateAlbedo = inputKind != TWK_DENOISER_RGB
        super().__init__(int(inputKind), int(iterations), sigmaColor, sigmaNormal, sigmaAlbedo, int(bool(demodulateAlbedo)), blendFactor)


class DenoiserVariance(C.Structure):
    """≙ TwkDenoiserVariance: parameters of twk_denoise_variance, the variance-guided, firefly-clamping mode of the filter.
    Without arguments: twk_denoiser_variance_defaults."""
    _fields_ = [("fireflyThreshold", C.c_float), ("sigmaLuminance", C.c_float)]

    def __init__(self, fireflyThreshold=3.0, sigmaLuminance=4.0):
        super().__init__(fireflyThreshold, sigmaLuminance)


class DenoiserGeometry(C.Structure):
    """≙ TwkDenoiserGeometry: parameters of twk_denoise_geometry, the geometry guide of the filter (plane and instance stops from
    the geometry AOV). Without arguments: twk_denoiser_geometry_defaults."""
    _fields_ = [("sigmaPosition", C.c_float), ("instanceStop", C.c_int)]

    def __init__(self, sigmaPosition=TWK_DENOISER_SIGMA_POSITION, instanceStop=0):
        super().__init__(sigmaPosition, int(bool(instanceStop)))


class Temporal(C.Structure):
    """≙ TwkTemporal: parameters of twk_temporal_accumulate. maxHistory: the cap, in samples, on what the history weighs;
    positionTolerance: a history tap belongs to the surface when its world position differs by at most this x the distance to
    the previous camera. Without arguments: twk_temporal_defaults."""
    _fields_ = [("maxHistory", C.c_int), ("positionTolerance", C.c_float)]

    def __init__(self, maxHistory=TWK_TEMPORAL_MAX_HISTORY, positionTolerance=TWK_TEMPORAL_POSITION_TOLERANCE):
        super().__init__(int(maxHistory), positionTolerance)


class TemporalRectify(C.Structure):
    """≙ TwkTemporalRectify: parameters of twk_temporal_accumulate_rectified. radius (1..4): the window of the paired test is
    (2 radius + 1)^2 pixels; minTaps (>= 2): fewer pixels of the centre's instance in the window and nothing is tested; gamma (>= 0):
    the standard errors a mean difference must exceed before the history is discounted. Without arguments:
    twk_temporal_rectify_defaults (provisional)."""
    _fields_ = [("radius", C.c_int), ("minTaps", C.c_int), ("gamma", C.c_float)]

    def __init__(self, radius=TWK_TEMPORAL_RECTIFY_RADIUS, minTaps=TWK_TEMPORAL_RECTIFY_MIN_TAPS, gamma=TWK_TEMPORAL_RECTIFY_GAMMA):
        super().__init__(int(radius), int(minTaps), gamma)


class TemporalFrame(C.Structure):
    """≙ TwkTemporalFrame: one frame's device buffers (colour, luminance moments, geometry AOV; ints or None) and its camera."""
    _fields_ = [("colour", C.c_void_p), ("moments", C.c_void_p), ("geometry", C.c_void_p), ("camera", CameraDefinition)]

    def __init__(self, colour=None, moments=None, geometry=None, camera=None):
        super().__init__(colour, moments, geometry, camera if camera is not None else CameraDefinition())


class InstanceMotion(C.Structure):
    """≙ TwkInstanceMotion (64 bytes): one instance's record of a motion table — previousFromCurrent, the row-major 3 x 4 matrix that
    carries a point of the instance in this frame to where it was in the history's frame, and moved (0: the instance is where it
    was, the matrix is not read). instance_motion(previous, current) fills one."""
    _fields_ = [("previousFromCurrent", C.c_float * 12), ("moved", C.c_uint), ("reserved", C.c_uint * 3)]


class InstanceCarry(C.Structure):
    """≙ TwkInstanceCarry (64 bytes): one instance's record beside its InstanceMotion for the previous-position plane
    (csrc/temporal_carry_device.h) — previousObjectToWorld, the instance's row-major 3 x 4 matrix as of the history's frame; deformed
    (0: nothing else is read); positionBase / indexBase, where its geometry's previous positions / indices begin."""
    _fields_ = [("previousObjectToWorld", C.c_float * 12), ("deformed", C.c_uint), ("positionBase", C.c_uint), ("indexBase", C.c_uint), ("reserved", C.c_uint)]


class Noise(C.Structure):
    """≙ TwkNoise: parameters of twk_estimate_noise. minSamples: a pixel with fewer samples is `unknown`; darkFloor: added to the
    mean the standard error is divided by. Without arguments: twk_noise_defaults."""
    _fields_ = [("minSamples", C.c_int), ("darkFloor", C.c_float)]

    def __init__(self, minSamples=TWK_DENOISER_MIN_SAMPLES, darkFloor=TWK_NOISE_DARK_FLOOR):
        super().__init__(int(minSamples), darkFloor)


class Adaptive(C.Structure):
    """≙ TwkAdaptive: parameters of twk_adaptive_select. An element is selected when its relative standard error (minSamples and
    darkFloor as in Noise) is above targetNoise or cannot be told yet, unless it is empty or its sample count has reached
    maxSamples. Without arguments: twk_adaptive_defaults."""
    _fields_ = [("targetNoise", C.c_float), ("minSamples", C.c_int), ("darkFloor", C.c_float), ("maxSamples", C.c_uint)]

    def __init__(self, targetNoise=TWK_ADAPTIVE_TARGET_NOISE, minSamples=TWK_DENOISER_MIN_SAMPLES, darkFloor=TWK_NOISE_DARK_FLOOR,
                 maxSamples=TWK_ADAPTIVE_MAX_SAMPLES):
        super().__init__(targetNoise, int(minSamples), darkFloor, int(maxSamples))


class AdaptivePlan(C.Structure):
    """≙ TwkAdaptivePlan: parameters of twk_adaptive_plan beside an Adaptive. A planned element gets the samples its noise estimate
    predicts, n (e / target)^2 - n, within [minBatch, maxBatch] (1 <= minBatch <= maxBatch <= 64) and the room maxSamples leaves; one
    without an estimate gets minBatch. Without arguments: twk_adaptive_plan_defaults (provisional)."""
    _fields_ = [("minBatch", C.c_uint32), ("maxBatch", C.c_uint32)]

    def __init__(self, minBatch=TWK_DENOISER_MIN_SAMPLES, maxBatch=64):
        super().__init__(int(minBatch), int(maxBatch))


class Cascade(C.Structure):
    """≙ TwkCascade: the firefly cascade's layers (2..8) and their thresholds start, start base, start base^2, ... (start > 0,
    base > 1). Without arguments: twk_cascade_defaults."""
    _fields_ = [("layers", C.c_int), ("start", C.c_float), ("base", C.c_float)]

    def __init__(self, layers=TWK_CASCADE_LAYERS, start=TWK_CASCADE_START, base=TWK_CASCADE_BASE):
        super().__init__(int(layers), start, base)


class CascadeResolve(C.Structure):
    """≙ TwkCascadeResolve: kappa (> 0), the sample count at which a layer is fully trusted. Without arguments:
    twk_cascade_resolve_defaults (provisional)."""
    _fields_ = [("kappa", C.c_float)]

    def __init__(self, kappa=TWK_CASCADE_KAPPA):
        super().__init__(kappa)


class AssemblySource(C.Structure):
    """≙ TwkAssemblySource: one source device's packed buffers for twk_assemble, device pointers (ints or None) indexed by
    TWK_PLANE_*. AssemblySource({TWK_PLANE_OUTPUT: ptr, ...}) fills the planes named."""
    _fields_ = [("plane", C.c_void_p * TWK_PLANE_COUNT)]

    def __init__(self, planes=None):
        super().__init__()
        for k, v in (planes or {}).items():
            self.plane[int(k)] = None if v is None else int(v)


TwkAssemblySource = AssemblySource


class NoiseSummary(C.Structure):
    """≙ TwkNoiseSummary: what twk_estimate_noise reduces a stream of luminance moments to (csrc/noise_device.h). valid / unknown /
    empty count the elements; the rest describes e, the relative standard error of the luminance mean, over the valid ones."""
    _fields_ = [("valid", C.c_uint64), ("unknown", C.c_uint64), ("empty", C.c_uint64), ("sumFixed", C.c_uint64),
                ("maxErrorBits", C.c_uint32), ("reserved", C.c_uint32), ("bins", C.c_uint32 * 256)]

    @property
    def histogram(self):
        """uint32 [256]: valid elements by the exponent and top three mantissa bits of e, 8 bins per octave from 2^-16 to 2^16."""
        return np.ctypeslib.as_array(self.bins).copy()

    @property
    def maxError(self):
        """The largest e (0.0 without a valid element)."""
        return float(np.array([self.maxErrorBits], np.uint32).view(np.float32)[0])

    @property
    def mean(self):
        """twk_noise_mean: the mean e of the valid elements (TwkError without one)."""
        m = C.c_float(0)
        check(lib.twk_noise_mean(C.byref(self), C.byref(m)))
        return m.value

    def quantile(self, q):
        """twk_noise_quantile: the upper edge of the histogram bin that holds the q quantile of e, q in (0, 1]: never below the
        true quantile, at most 9/8 of it inside the histogram's range (TwkError without a valid element)."""
        e = C.c_float(0)
        check(lib.twk_noise_quantile(C.byref(self), C.c_float(q), C.byref(e)))
        return e.value

    def merge(self, other):
        """twk_noise_merge: folds the summary of a disjoint set of elements (another device's tiles) into this one; returns self."""
        check(lib.twk_noise_merge(C.byref(self), C.byref(other)))
        return self


class LaunchStats(C.Structure):
    _fields_ = [("radianceRays", C.c_uint64), ("shadowRays", C.c_uint64), ("nodesVisited", C.c_uint64),
                ("trianglesTested", C.c_uint64), ("instancesEntered", C.c_uint64), ("shadedHits", C.c_uint64),
                ("missed", C.c_uint64), ("maxNodesPerRay", C.c_uint64), ("tailRays", C.c_uint64),
                ("tailNodesVisited", C.c_uint64), ("tailTrianglesTested", C.c_uint64), ("tailInstancesEntered", C.c_uint64),
                ("overflowRays", C.c_uint64),
                ("nodeWaveSteps", C.c_uint64), ("triangleWaveSteps", C.c_uint64), ("leafWaveSteps", C.c_uint64),
                ("cachedNodesVisited", C.c_uint64), ("droppedStackPushes", C.c_uint64), ("waveCycles", C.c_uint64 * 6),
                ("shadePhaseWaveSteps", C.c_uint64 * 24), ("shadePhaseLanes", C.c_uint64 * 24), ("shadePhaseCycles", C.c_uint64 * 24)]


class AccelerationInfo(C.Structure):
    _fields_ = [("root", C.c_int), ("twoLevel", C.c_int), ("numNodes", C.c_uint64), ("numTriangleSlots", C.c_uint64), ("numInstances", C.c_uint64),
                ("root2", C.c_int), ("nodeFloats", C.c_int)]


class BuildInfo(C.Structure):
    _fields_ = [("quality", C.c_int), ("trees", C.c_int), ("sahInnerCost", C.c_double), ("sahLeafCost", C.c_double),
                ("buildMilliseconds", C.c_double), ("triangleSlots", C.c_uint64), ("nodes", C.c_uint64),
                ("instances", C.c_uint64), ("flattenedInstances", C.c_uint64), ("maxTraversalDepth", C.c_uint64),
                ("directLeafInstances", C.c_uint64), ("traceBlocksPerCU", C.c_uint64),
                ("wide8Nodes", C.c_uint64), ("wide8Levels", C.c_uint64),
                ("pairLeaves", C.c_uint64), ("pairTriangles", C.c_uint64)]


TWK_UPDATE_FULL, TWK_UPDATE_SELECTIVE = 0, 1  # twk_set_update_mode (include/tweeker_hip.h "Selective instance updates")


class UpdateInfo(C.Structure):
    """≙ TwkUpdateInfo: what the last instance-transform update of a handle did (twk_get_update_info)."""
    _fields_ = [("selective", C.c_int), ("instancesMoved", C.c_int), ("treesRebuilt", C.c_int), ("topLevelRebuilt", C.c_int),
                ("nodesRequantised", C.c_uint64), ("slotsRewritten", C.c_uint64), ("instanceRecordsUploaded", C.c_uint64),
                ("keptBytes", C.c_uint64), ("milliseconds", C.c_double)]


class RefitInfo(C.Structure):
    """≙ TwkRefitInfo: what the last refit of a handle did (twk_get_refit_info)."""
    _fields_ = [("treesRefit", C.c_int), ("treesRebuilt", C.c_int), ("topLevelRebuilt", C.c_int), ("refitsSinceBuild", C.c_int),
                ("nodesRefit", C.c_uint64), ("slotsRewritten", C.c_uint64), ("sahBuilt", C.c_double), ("sahNow", C.c_double),
                ("milliseconds", C.c_double)]


class RefitBatchPlan(C.Structure):
    """≙ TwkRefitBatchPlan: the totals of a batched refit's block plan (twk_refit_batch_plan_host)."""
    _fields_ = [("trees", C.c_int), ("nodeBlocks", C.c_int), ("slotBlocks", C.c_int), ("blockThreads", C.c_int),
                ("nodes", C.c_uint64), ("slots", C.c_uint64)]


class VertexSource(C.Structure):
    """≙ TwkVertexSource: vertices that live on the device (twk_update_geometry_vertices_device, twk_refit_geometry_vertices_device):
    exactly one of attributes (48-byte records) and positions (x, y, z floats, positionStride bytes apart; 0 means 12) is set."""
    _fields_ = [("attributes", C.c_void_p), ("positions", C.c_void_p), ("positionStride", C.c_size_t), ("recomputeFrames", C.c_uint),
                ("reserved", C.c_uint * 3)]


class GeometryEdit(C.Structure):
    """≙ TwkGeometryEdit: one geometry entry of twk_refit_scene — host records (attributes) or a device source (source: a pointer to a
    VertexSource), exactly one of the two."""
    _fields_ = [("idGeometry", C.c_int32), ("reserved", C.c_uint32), ("numVertices", C.c_uint64), ("attributes", C.c_void_p), ("source", C.POINTER(VertexSource))]


class SceneRefitPlan(C.Structure):
    """≙ TwkSceneRefitPlan: the totals of a twk_refit_scene call's batch (twk_scene_refit_plan_host)."""
    _fields_ = [("trees", C.c_int), ("nodeBlocks", C.c_int), ("slotBlocks", C.c_int), ("blockThreads", C.c_int),
                ("directLeaves", C.c_int), ("boxes", C.c_int), ("topLevelRebuilt", C.c_int), ("reserved", C.c_int),
                ("nodes", C.c_uint64), ("slots", C.c_uint64), ("slotsRewritten", C.c_uint64), ("slotBytes", C.c_uint64)]


class UpdatePlan(C.Structure):
    """≙ TwkUpdatePlan: the layout of a scene and what a selective update of some of its instances touches (twk_update_plan_host)."""
    _fields_ = [("instances", C.c_int), ("flattenedInstances", C.c_int), ("directLeafInstances", C.c_int), ("enteredGeometries", C.c_int),
                ("treesRebuilt", C.c_int), ("topLevelRebuilt", C.c_int), ("numRanges", C.c_int), ("tlasBase", C.c_int),
                ("nodes", C.c_uint64), ("triangleSlots", C.c_uint64), ("nodesRequantised", C.c_uint64), ("slotsRewritten", C.c_uint64)]


class AppInfo(C.Structure):
    _fields_ = [("strategy", C.c_int), ("devicesMask", C.c_int), ("light", C.c_int), ("miss", C.c_int),
                ("lensShader", C.c_int), ("samplesSqrt", C.c_int), ("resolution", i2), ("tileSize", i2),
                ("pathLengths", i2), ("epsilonFactor", C.c_float), ("envRotation", C.c_float),
                ("clockFactor", C.c_float), ("center", f3), ("phi", C.c_float), ("theta", C.c_float),
                ("fov", C.c_float), ("distance", C.c_float), ("numCameras", C.c_int), ("numLights", C.c_int),
                ("numMaterials", C.c_int), ("numGeometries", C.c_int), ("numInstances", C.c_int),
                ("shaderVariant", C.c_int), ("nextEventEstimation", C.c_int), ("debugExceptions", C.c_int)]


# Every symbol include/tweeker_hip.h declares; tests/test_cabi_symbols.py checks header == this list == the .so.
SYMBOLS = [
    "twk_last_error", "twk_abi_version", "twk_device_count", "twk_device_create", "twk_device_destroy",
    "twk_set_state", "twk_init_cameras", "twk_init_lights", "twk_init_materials", "twk_update_camera",
    "twk_update_light", "twk_update_material", "twk_init_texture", "twk_add_geometry", "twk_add_instance",
    "twk_build", "twk_clear_scene", "twk_set_flatten_policy", "twk_set_build_quality", "twk_get_build_info", "twk_get_stream_layout", "twk_launch", "twk_sync", "twk_set_launch_batch", "twk_reserve_launch_batch", "twk_get_launch_width", "twk_read_output",
    "twk_set_shader_variant", "twk_enable_aov", "twk_read_aov", "twk_set_time_view", "twk_set_next_event_estimation", "twk_set_debug_exceptions", "twk_get_output_device_pointer", "twk_set_output_device_pointer", "twk_set_shared_frame", "twk_compositor", "twk_tonemap", "twk_profile_enable",
    "twk_set_output_format", "twk_get_output_format", "twk_read_output_raw", "twk_read_aov_raw", "twk_compositor_half", "twk_tonemap_half",
    "twk_app_get_output_format",
    "twk_denoiser_defaults", "twk_denoise", "twk_read_denoised", "twk_read_denoised_raw", "twk_get_denoised_device_pointer", "twk_app_get_denoiser",
    "twk_denoiser_variance_defaults", "twk_denoise_variance", "twk_app_get_denoiser_variance",
    "twk_enable_moments", "twk_read_moments", "twk_get_moments_device_pointer", "twk_debug_read_path_radiance", "twk_denoise_variance_sampled", "twk_app_get_denoiser_sampled",
    "twk_denoiser_geometry_defaults", "twk_denoise_geometry", "twk_denoise_geometry_host", "twk_app_get_denoiser_geometry",
    "twk_set_sample_offset", "twk_enable_geometry", "twk_render_geometry", "twk_read_geometry", "twk_get_geometry_device_pointer",
    "twk_temporal_defaults", "twk_temporal_accumulate", "twk_temporal_reset", "twk_get_temporal_device_pointers", "twk_read_temporal", "twk_read_temporal_moments",
    "twk_noise_defaults", "twk_estimate_noise", "twk_read_noise", "twk_noise_merge", "twk_noise_mean", "twk_noise_quantile", "twk_app_get_target_noise",
    "twk_enable_adaptive", "twk_adaptive_defaults", "twk_adaptive_select", "twk_adaptive_select_host", "twk_launch_adaptive", "twk_read_sample_counts",
    "twk_get_sample_counts_device_pointer", "twk_read_active", "twk_app_get_adaptive",
    "twk_adaptive_plan_defaults", "twk_adaptive_plan", "twk_adaptive_plan_host", "twk_launch_adaptive_planned", "twk_read_plan", "twk_app_get_adaptive_plan",
    "twk_cascade_defaults", "twk_cascade_resolve_defaults", "twk_enable_cascade", "twk_read_cascade", "twk_get_cascade_device_pointer", "twk_cascade_resolve",
    "twk_get_resolved_device_pointer", "twk_read_resolved", "twk_cascade_fold_host", "twk_cascade_resolve_host", "twk_app_get_cascade",
    "twk_temporal_rectify_defaults", "twk_temporal_accumulate_rectified", "twk_get_temporal_trust_device_pointer", "twk_read_temporal_trust",
    "twk_temporal_accumulate_cascade_trusted", "twk_temporal_accumulate_assembled_rectified", "twk_temporal_rectify_host", "twk_temporal_cascade_trusted_host",
    "twk_temporal_accumulate_cascade", "twk_temporal_enable_cascade", "twk_get_temporal_cascade_device_pointer", "twk_read_temporal_cascade", "twk_temporal_cascade_host",
    "twk_instance_motion", "twk_update_instance_transform", "twk_get_instance_transform", "twk_temporal_accumulate_moving", "twk_temporal_accumulate_cascade_moving",
    "twk_temporal_moving_host", "twk_temporal_cascade_moving_host", "twk_read_temporal_motion", "twk_app_get_temporal_motion",
    "twk_set_update_mode", "twk_update_instance_transforms", "twk_get_update_info", "twk_update_plan_host", "twk_app_get_selective_update",
    "twk_update_geometry_vertices", "twk_get_geometry_deformed", "twk_vertex_update_plan_host", "twk_render_geometry_motion", "twk_get_previous_position_device_pointer",
    "twk_read_previous_positions", "twk_previous_positions_host",
    "twk_refit_geometry_vertices", "twk_get_refit_info", "twk_refit_tree_host", "twk_debug_read_kept_build",
    "twk_refit_instance_transform", "twk_refit_instance_transforms", "twk_refit_batch_plan_host",
    "twk_update_geometry_vertices_device", "twk_refit_geometry_vertices_device", "twk_vertex_frames_host", "twk_read_geometry_vertices",
    "twk_refit_scene", "twk_scene_refit_plan_host",
    "twk_enable_emitter_motion", "twk_get_emitter_motion", "twk_get_light", "twk_light_moved_host",
    "twk_temporal_accumulate_carried", "twk_temporal_accumulate_cascade_carried", "twk_temporal_carried_host", "twk_temporal_cascade_carried_host",
    "twk_assemble", "twk_assemble_devices", "twk_get_assembled_device_pointer", "twk_read_assembled", "twk_assemble_host", "twk_app_get_tile_assembly",
    "twk_render_geometry_tile", "twk_assemble_with_geometry", "twk_assemble_devices_with_geometry", "twk_get_assembled_geometry_device_pointer",
    "twk_read_assembled_geometry", "twk_temporal_accumulate_assembled", "twk_app_get_temporal", "twk_app_get_temporal_rectify",
    "twk_profile_reset", "twk_profile_get", "twk_stats_enable", "twk_stats_get", "twk_stream_peak_gbps", "twk_gather_peak",
    "twk_debug_capture", "twk_debug_shade_builds", "twk_debug_shade_build_slots", "twk_debug_read_first_hits", "twk_trace_rays", "twk_debug_trace_queue", "twk_debug_read_acceleration", "twk_debug_snapshot_scene", "twk_debug_math", "twk_debug_exact_division",
    "twk_app_create", "twk_app_create_from_strings", "twk_app_destroy", "twk_app_info", "twk_app_set_resolution",
    "twk_app_get_state", "twk_app_get_cameras", "twk_app_get_lights", "twk_app_get_materials",
    "twk_app_get_geometry_sizes", "twk_app_get_geometry", "twk_app_get_instance", "twk_app_init_device",
    "twk_app_system_description", "twk_app_get_tonemapper", "twk_app_screenshot_path", "twk_load_image", "twk_app_get_environment",
    "twk_write_png_rgb8", "twk_write_hdr_rgba32f",
    "twk_mesh_plane", "twk_mesh_box", "twk_mesh_sphere", "twk_mesh_torus", "twk_mesh_parallelogram",
    "twk_camera_frustum", "twk_tile_column", "twk_launch_width", "twk_parse_tokens",
]

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). tweeker_raytracer_amd has no CPU fallback.")

lib = C.CDLL(LIB_PATH)
lib.twk_last_error.restype = C.c_char_p
for _name in SYMBOLS:
    if _name != "twk_last_error":
        getattr(lib, _name).restype = C.c_int


def check(code):
    if code != TWK_SUCCESS:
        raise TwkError(code, (lib.twk_last_error() or b"").decode("utf-8", "replace"))
    return code

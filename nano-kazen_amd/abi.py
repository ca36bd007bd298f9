"""ctypes mirror of include/kazen_mi355x.h and the loader of libkazen_mi355x.so.

Plumbing only: every structure here is a field-for-field copy of the C header (which cites
the reference interface each one replaces). The loader FAILS LOUDLY when the HIP extension
is missing: there is no CPU fallback in the product path.
"""
import ctypes as C
import os

KZ_ABI_VERSION = 6

KZ_OK, KZ_ERR_INVALID_ARG, KZ_ERR_UNSUPPORTED, KZ_ERR_NO_DEVICE, KZ_ERR_HIP, KZ_ERR_STATE, KZ_ERR_OOM = range(7)
KZ_BSDF_DIFFUSE, KZ_BSDF_KAZENSTANDARD, KZ_BSDF_MIRROR, KZ_BSDF_DIELECTRIC = 0, 1, 2, 3
KZ_BSDF_GGX, KZ_BSDF_ROUGHCONDUCTOR, KZ_BSDF_ROUGHPLASTIC, KZ_BSDF_ROUGHDIELECTRIC, KZ_BSDF_NORMALMAP = 4, 5, 6, 7, 8
KZ_TEX_CONSTANT, KZ_TEX_IMAGE, KZ_TEX_COLORRAMP, KZ_TEX_BLEND = 0, 1, 2, 3
KZ_BLEND_MIX, KZ_BLEND_MULTIPLY, KZ_BLEND_NONE = 0, 1, 2
KZ_PIXEL_U8, KZ_PIXEL_F32 = 0, 1
KZ_TEX_MAX_DEPTH = 8
KZ_SAMPLER_INDEPENDENT, KZ_SAMPLER_PMJ02BN, KZ_SAMPLER_STRATIFIED, KZ_SAMPLER_CORRELATED = 0, 1, 2, 3
KZ_CAMERA_PERSPECTIVE, KZ_CAMERA_THINLENS = 0, 1
KZ_INTEGRATOR_PATH_MIS, KZ_INTEGRATOR_NORMALS, KZ_INTEGRATOR_AO, KZ_INTEGRATOR_PATH_MATS = 0, 1, 2, 3
KZ_FILTER_GAUSSIAN, KZ_FILTER_MITCHELL, KZ_FILTER_TENT, KZ_FILTER_BOX = 0, 1, 2, 3
KZ_FILTER_RESOLUTION = 32
KZ_PMJ02BN_SETS, KZ_PMJ02BN_SAMPLES = 5, 65536
KZ_BLUENOISE_TEXTURES, KZ_BLUENOISE_RES = 48, 128

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
u16p = C.POINTER(C.c_uint16)


class KzBSDF(C.Structure):
    _fields_ = [("type", C.c_int32), ("albedo", C.c_float * 3), ("baseColor", C.c_float * 3),
                ("roughness", C.c_float), ("metallic", C.c_float), ("anisotropy", C.c_float),
                ("specular", C.c_float), ("specularTint", C.c_float), ("clearcoat", C.c_float),
                ("clearcoatRoughness", C.c_float), ("sheen", C.c_float), ("sheenTint", C.c_float),
                ("intIOR", C.c_float), ("extIOR", C.c_float), ("alpha", C.c_float), ("condEta", C.c_float * 3),
                ("condK", C.c_float * 3), ("albedoTex", C.c_int32), ("roughnessTex", C.c_int32), ("metallicTex", C.c_int32),
                ("normalTex", C.c_int32), ("nested", C.c_int32), ("alphaResolved", C.c_int32), ("pad_", C.c_int32)]


class KzImage(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("format", C.c_int32)]


class KzTexture(C.Structure):
    _fields_ = [("type", C.c_int32), ("color", C.c_float * 3), ("image", C.c_int32), ("scale", C.c_float), ("srgb", C.c_int32),
                ("rampMin", C.c_float), ("rampMax", C.c_float), ("blendMode", C.c_int32), ("child", C.c_int32 * 3), ("filter", C.c_int32), ("pad_", C.c_int32 * 2)]


class KzLight(C.Structure):
    _fields_ = [("color", C.c_float * 3), ("intensity", C.c_float), ("primaryVisibility", C.c_int32)]


class KzMesh(C.Structure):
    _fields_ = [("V", f32p), ("N", f32p), ("UV", f32p), ("F", u32p), ("nV", C.c_uint32), ("nF", C.c_uint32),
                ("bsdf", C.c_int32), ("light", C.c_int32)]


class KzFilter(C.Structure):
    _fields_ = [("type", C.c_int32), ("radius", C.c_float), ("stddev", C.c_float), ("B", C.c_float), ("C", C.c_float)]


class KzCamera(C.Structure):
    _fields_ = [("type", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("toWorld", C.c_float * 16),
                ("fov", C.c_float), ("nearClip", C.c_float), ("farClip", C.c_float),
                ("apertureRadius", C.c_float), ("focusDistance", C.c_float),
                ("sampleToCamera", f32p), ("rfilter", KzFilter)]


class KzSampler(C.Structure):
    _fields_ = [("type", C.c_int32), ("sampleCount", C.c_uint32), ("resolution", C.c_int32), ("pad_", C.c_int32), ("seed", C.c_uint64),
                ("pmj02bnSamples", u32p), ("blueNoise", u16p)]


class KzIntegrator(C.Structure):
    _fields_ = [("type", C.c_int32), ("maxDepth", C.c_int32), ("traceBias", C.c_float),
                ("regularization", C.c_int32), ("accumulatedRoughness", C.c_float)]


class KzBackground(C.Structure):
    _fields_ = [("present", C.c_int32), ("color", C.c_float * 3), ("intensity", C.c_float), ("texture", C.c_int32)]


class KzSceneDesc(C.Structure):
    _fields_ = [("abiVersion", C.c_uint32),
                ("meshes", C.POINTER(KzMesh)), ("nMeshes", C.c_uint32),
                ("bsdfs", C.POINTER(KzBSDF)), ("nBsdfs", C.c_uint32),
                ("lights", C.POINTER(KzLight)), ("nLights", C.c_uint32),
                ("camera", KzCamera), ("sampler", KzSampler), ("integrator", KzIntegrator),
                ("background", KzBackground),
                ("textures", C.POINTER(KzTexture)), ("nTextures", C.c_uint32),
                ("images", C.POINTER(KzImage)), ("nImages", C.c_uint32)]


class KzTile(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


class KzTuning(C.Structure):
    # dev0 .. dev5: reserved words (kazen_mi355x.h); the values that once selected kernels of rejected experiments are refused with KZ_ERR_UNSUPPORTED
    _fields_ = [("refill", C.c_int32), ("postpone", C.c_int32), ("batch", C.c_int32), ("traceBlocksPerCU", C.c_int32),
                ("shadeBlocksPerCU", C.c_int32), ("ldsStack", C.c_int32), ("dev0", C.c_int32), ("packetPrimary", C.c_int32),
                ("dev1", C.c_int32), ("dev2", C.c_int32), ("filmGather", C.c_int32), ("dev3", C.c_int32), ("sppPerPass", C.c_int32), ("dev4", C.c_int32),
                ("dev5", C.c_int32), ("streamPriority", C.c_int32)]


class KzTileDealer(C.Structure):
    _fields_ = [("counter", u32p), ("batchTiles", C.c_uint32), ("takers", C.c_uint32), ("taken", u32p), ("takenCap", C.c_uint32), ("nTaken", u32p), ("agreed", u32p)]


class KzRenderOpts(C.Structure):
    _fields_ = [("sampleBegin", C.c_uint32), ("sampleEnd", C.c_uint32), ("tiles", C.POINTER(KzTile)),
                ("nTiles", C.c_uint32), ("pipeline", C.c_int32), ("accumulate", C.c_int32), ("stream", C.c_void_p),
                ("device", C.c_int32), ("passesInFlight", C.c_int32), ("passItems", C.c_uint64), ("maxStateBytes", C.c_uint64),
                ("tune", KzTuning), ("tileDealing", C.c_int32), ("packedOutput", C.c_int32), ("dealer", C.POINTER(KzTileDealer)),
                ("shadowBeside", C.c_int32), ("passHalves", C.c_int32)]


class KzPassInfo(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("passesInFlight", C.c_uint32), ("itemsPerPass", C.c_uint64), ("sppPerPass", C.c_uint32),
                ("pixels", C.c_uint32), ("stateBytes", C.c_uint64), ("pixelsPerPass", C.c_uint32), ("shadowBeside", C.c_uint32),
                ("firstPassItems", C.c_uint64), ("largestPassItems", C.c_uint64), ("contextItems", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class KzPassModeInfo(C.Structure):
    _fields_ = [("kept", C.c_int32), ("timedPasses", C.c_uint32), ("items", C.c_uint64), ("msOneStream", C.c_float * 2), ("msShadowBeside", C.c_float), ("msHalves", C.c_float)]


class KzPlanQuery(C.Structure):
    _fields_ = [("pipeline", C.c_int32), ("nPix", C.c_uint32), ("sampleBegin", C.c_uint32), ("sampleEnd", C.c_uint32), ("passItems", C.c_uint64),
                ("passesInFlight", C.c_int32), ("sppPerPass", C.c_int32), ("limitBytes", C.c_uint64), ("bytesPerItem", C.c_uint64), ("dealer", C.c_int32),
                ("takers", C.c_uint32), ("batchTiles", C.c_uint32), ("nTiles", C.c_uint32), ("tilePixOffset", u32p), ("heldItems", C.c_uint64)]


class KzPlanAnswer(C.Structure):
    _fields_ = [("autoShape", C.c_int32), ("nCtx", C.c_int32), ("multi", C.c_int32), ("grow", C.c_int32), ("S", C.c_uint32), ("pixPerPass", C.c_uint32),
                ("batchTiles", C.c_uint32), ("nPixSet", C.c_uint32), ("nPasses", C.c_uint32), ("need", C.c_uint64), ("wantItems", C.c_uint64),
                ("minStart", C.c_uint64), ("graceMs", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KzPassModeQuery(C.Structure):
    _fields_ = [("items", C.c_uint64), ("nPixPass", C.c_uint32), ("shadowBeside", C.c_int32), ("passHalves", C.c_int32), ("pipeline", C.c_int32),
                ("multi", C.c_int32), ("dealer", C.c_int32), ("statsOn", C.c_int32), ("pathMis", C.c_int32), ("nLights", C.c_int32), ("maxDepth", C.c_int32),
                ("reset", C.c_int32), ("launch", C.c_int32), ("ms", C.c_float * 4)]


class KzPassModeState(C.Structure):
    _fields_ = [("kept", C.c_int32), ("launched", C.c_int32), ("items", C.c_uint64 * 4), ("ms", C.c_float * 4)]


class KzPassModeAnswer(C.Structure):
    _fields_ = [("shadowBeside", C.c_int32), ("halves", C.c_int32), ("probe", C.c_int32), ("beside", C.c_int32), ("besideSecondHalf", C.c_int32),
                ("firstHalfPixels", C.c_uint32), ("settled", C.c_int32)]


class KzStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("nodeVisits", C.c_uint64), ("triTests", C.c_uint64),
                ("shadedHits", C.c_uint64), ("lightSamples", C.c_uint64), ("droppedSamples", C.c_uint64),
                ("beamPixels", C.c_uint64), ("beamListEntries", C.c_uint64), ("beamCompletePixels", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class KzHit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("mesh", C.c_int32), ("prim", C.c_int32),
                ("p", C.c_float * 3), ("uv", C.c_float * 2), ("sh_s", C.c_float * 3), ("sh_t", C.c_float * 3),
                ("sh_n", C.c_float * 3), ("geo_n", C.c_float * 3)]


class KzTraceWfOpts(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("stats", C.c_int32), ("refill", C.c_int32), ("postpone", C.c_int32), ("batch", C.c_int32), ("ldsStack", C.c_int32),
                ("gridBlocks", C.c_int32), ("packetBatch", C.c_int32)]


class KzTraceWfHit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("gid", C.c_uint32), ("mesh", C.c_int32), ("prim", C.c_int32)]


class KzTraceWfInfo(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodeVisits", C.c_uint64), ("triTests", C.c_uint64), ("nQueueB", C.c_uint32), ("nFirstHitsOnInvisibleLight", C.c_uint32),
                ("gridBlocks", C.c_uint32), ("ldsStack", C.c_uint32), ("stackBound", C.c_uint32), ("ovfRows", C.c_uint32), ("ovfRowsTouched", C.c_uint32),
                ("shadowFast", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class KzVertexUpdate(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("nV", C.c_uint32), ("V", f32p), ("N", f32p)]


class KzBsdfUpdate(C.Structure):
    _fields_ = [("row", C.c_uint32), ("bsdf", KzBSDF)]


class KzLightUpdate(C.Structure):
    _fields_ = [("light", C.c_uint32), ("value", KzLight)]


class KzTransformUpdate(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("toWorld", C.c_float * 16)]


class KzDenoiseOpts(C.Structure):
    # include/kazen_mi355x_denoise.h: 32 bytes, a zero field means its default
    _fields_ = [("iterations", C.c_uint32), ("guides", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float), ("sigmaDepth", C.c_float), ("sigmaAlbedo", C.c_float)]


class KzVarianceOpts(C.Structure):
    # include/kazen_mi355x_variance.h: 16 bytes, a zero field means its default
    _fields_ = [("sigmaVariance", C.c_float), ("samples", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class KzTemporalView(C.Structure):
    # include/kazen_mi355x_temporal.h: 96 bytes, a pinhole view - the direction through (sx, sy) is a + sx u + sy v; inv: the inverse of the matrix with columns (u, v, a)
    _fields_ = [("o", C.c_float * 3), ("a", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("inv", C.c_float * 9), ("reserved", C.c_float * 3)]


class KzTemporalOpts(C.Structure):
    # include/kazen_mi355x_temporal.h: 32 bytes, a zero field means its default
    _fields_ = [("depthTolerance", C.c_float), ("normalTolerance", C.c_float), ("maxHistory", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class KzMotionRow(C.Structure):
    # include/kazen_mi355x_motion.h: 96 bytes - where a point of a mesh was when the history was stored: d (3 x 4) = H C^-1, n (3 x 3) its linear part's inverse transpose
    _fields_ = [("d", C.c_float * 12), ("n", C.c_float * 9), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class KzResponsiveOpts(C.Structure):
    # include/kazen_mi355x_responsive.h: 32 bytes, a zero field means its default
    _fields_ = [("fastHistory", C.c_uint32), ("clampSigma", C.c_float), ("radius", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class KzMatteTexel(C.Structure):
    _fields_ = [("id", C.c_uint32 * 7), ("count", C.c_uint32 * 7), ("other", C.c_uint32), ("miss", C.c_uint32)]


# the same 64 bytes as a numpy record: what Scene.matte() and matte_accumulate_items() hand back
MATTE_DTYPE = [("id", "<u4", (7,)), ("count", "<u4", (7,)), ("other", "<u4"), ("miss", "<u4")]


class KzAdaptiveOpts(C.Structure):
    # include_ext/kazen_mi355x_adaptive.h: 32 bytes; threshold has no default, a zero in any other field means its default
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("minSamples", C.c_uint32), ("maxSamples", C.c_uint32), ("step", C.c_uint32), ("block", C.c_uint32),
                ("outlierPermille", C.c_uint32), ("flags", C.c_uint32)]


class KzAdaptiveBlock(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("noisy", C.c_uint32), ("valid", C.c_uint32), ("flags", C.c_uint32)]


class KzAdaptiveInfo(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("blocks", C.c_uint32), ("converged", C.c_uint32), ("atCap", C.c_uint32), ("samples", C.c_uint64), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the same 16 bytes as a numpy record: what Scene.adaptive_blocks() and adaptive_classify_films() hand back
ADAPTIVE_BLOCK_DTYPE = [("samples", "<u4"), ("noisy", "<u4"), ("valid", "<u4"), ("flags", "<u4")]


class KzBvhInfo(C.Structure):
    _fields_ = [("nNodes", C.c_uint32), ("nLeaves", C.c_uint32), ("nTris", C.c_uint32), ("maxDepth", C.c_uint32),
                ("maxLeafSize", C.c_uint32), ("sahCost", C.c_float), ("buildSeconds", C.c_double)]


# every symbol include/kazen_mi355x.h (the product surface, PRODUCT_EXPORTS) and include/kazen_mi355x_dev.h declare (checked by tests/test_abi_cpu.py)
PRODUCT_EXPORTS = ["kz_scene_create", "kz_scene_destroy", "kz_scene_upload", "kz_scene_evict", "kz_render", "kz_render_tiles", "kz_render_multi", "kz_deal_tiles",
                   "kz_tiles_packed_floats", "kz_film_download_tiles", "kz_film_merge_tiles", "kz_film_merge_rects", "kz_film_download", "kz_film_clear", "kz_film_dims", "kz_film_to_rgb",
                   "kz_film_to_srgb8", "kz_sync", "kz_last_error", "kz_abi_version", "kz_device_count", "kz_device_trim"]
EXPORTS = ["kz_scene_create", "kz_scene_destroy", "kz_scene_bvh_info", "kz_scene_upload", "kz_render",
           "kz_film_download", "kz_film_clear", "kz_film_dims", "kz_film_to_rgb", "kz_trace_rays",
           "kz_set_stats", "kz_get_stats", "kz_sync", "kz_last_kernel_ms", "kz_last_error", "kz_abi_version",
           "kz_device_count", "kz_render_samples", "kz_bsdf_query", "kz_scene_sample_count", "kz_last_stage_ms", "kz_texture_query", "kz_film_to_srgb8",
           "kz_scene_evict", "kz_scene_devices", "kz_render_tiles", "kz_render_multi", "kz_deal_tiles", "kz_film_merge", "kz_film_download_on",
           "kz_film_clear_on", "kz_sync_on", "kz_last_pass_info", "kz_device_mem_info", "kz_camera_rays", "kz_light_query", "kz_kat_exact_math", "kz_kat_permute", "kz_kat_fresnel", "kz_kat_math", "kz_build_flags",
           "kz_tiles_packed_floats", "kz_film_download_tiles", "kz_film_merge_tiles", "kz_film_merge_rects", "kz_device_trim", "kz_kat_dpdf", "kz_kat_pow4", "kz_last_grow_note",
           "kz_plan_passes", "kz_plan_schedule", "kz_plan_pass_mode", "kz_pass_mode_info", "kz_scene_table", "kz_trace_rays_wf"]
# what include/kazen_mi355x_edit.h declares (checked by tests/test_scene_edit_cpu.py): editing a scene that already exists
EDIT_EXPORTS = ["kz_scene_set_camera", "kz_scene_set_vertices", "kz_scene_set_bsdfs", "kz_scene_set_lights", "kz_scene_set_transforms"]
# what include/kazen_mi355x_aov.h declares (checked by tests/test_aov_cpu.py): albedo / normal / depth feature films beside the picture
AOV_EXPORTS = ["kz_scene_set_aovs", "kz_scene_aovs", "kz_aov_download", "kz_aov_download_on", "kz_aov_info", "kz_aov_samples"]
KZ_AOV_ALBEDO, KZ_AOV_NORMAL, KZ_AOV_DEPTH, KZ_AOV_ALL = 1, 2, 4, 7
AOV_BITS = {"albedo": KZ_AOV_ALBEDO, "normal": KZ_AOV_NORMAL, "depth": KZ_AOV_DEPTH}
# what include/kazen_mi355x_denoise.h declares (checked by tests/test_denoise_cpu.py): the picture denoised on the device, guided by its feature films
DENOISE_EXPORTS = ["kz_denoise", "kz_denoise_on", "kz_denoise_download", "kz_denoise_to_srgb8", "kz_denoise_info", "kz_denoise_release", "kz_denoise_films"]
KZ_DENOISE_NO_DEMODULATE, KZ_DENOISE_NO_GUIDES, KZ_DENOISE_MAX_ITERATIONS = 1, 2, 8
# what include/kazen_mi355x_variance.h declares (checked by tests/test_variance_cpu.py): a second-moment film beside the picture's and the denoiser guided by its variance
VARIANCE_EXPORTS = ["kz_scene_set_variance", "kz_scene_variance", "kz_variance_download", "kz_variance_info", "kz_denoise_variance", "kz_denoise_variance_films"]
KZ_VARIANCE_OFF, KZ_VARIANCE_ON, KZ_VARIANCE_TWO_LAUNCHES, KZ_VARIANCE_ONE_PASS = 0, 1, 2, 3
# what include/kazen_mi355x_temporal.h declares (checked by tests/test_temporal_cpu.py): the denoiser's history, reprojected across camera edits and blended in
TEMPORAL_EXPORTS = ["kz_temporal_view", "kz_denoise_temporal", "kz_temporal_info", "kz_temporal_reset", "kz_temporal_download", "kz_denoise_temporal_films"]
# what include/kazen_mi355x_motion.h declares (checked by tests/test_motion_cpu.py): the history kept across kz_scene_set_transforms - per-mesh rows and a mesh id per pixel
MOTION_EXPORTS = ["kz_motion_rows", "kz_motion_ids", "kz_denoise_motion", "kz_denoise_motion_films", "kz_motion_info"]
KZ_MOTION_STATIC, KZ_MOTION_UNTRACKED, KZ_MOTION_MISS = 1, 2, 0xFFFFFFFF
# what include/kazen_mi355x_responsive.h declares (checked by tests/test_responsive_cpu.py): a fast history beside the long one, which is clamped to it where the light moved
RESPONSIVE_EXPORTS = ["kz_denoise_responsive", "kz_denoise_responsive_films", "kz_responsive_download", "kz_responsive_info"]
KZ_RESPONSIVE_CLAMP_OFF = 1
# what include_ext/kazen_mi355x_matte.h declares (checked by tests/test_matte_cpu.py): ID mattes - per pixel (mesh or BSDF-row id, sample count) slots beside the picture
MATTE_EXPORTS = ["kz_scene_set_mattes", "kz_scene_mattes", "kz_matte_download", "kz_matte_download_on", "kz_matte_layer", "kz_matte_top", "kz_matte_info",
                 "kz_matte_accumulate_items"]
KZ_MATTE_MESH, KZ_MATTE_BSDF, KZ_MATTE_ALL, KZ_MATTE_SLOTS, KZ_MATTE_NONE = 1, 2, 3, 7, 0xFFFFFFFF
MATTE_BITS = {"mesh": KZ_MATTE_MESH, "bsdf": KZ_MATTE_BSDF}
# what include_ext/kazen_mi355x_adaptive.h declares (checked by tests/test_adaptive_cpu.py): adaptive sampling - rounds over the blocks whose variance has not converged
ADAPTIVE_EXPORTS = ["kz_render_adaptive", "kz_adaptive_blocks", "kz_adaptive_counts", "kz_adaptive_info", "kz_adaptive_classify_films", "kz_adaptive_schedule",
                    "kz_adaptive_tiles", "kz_adaptive_stage_ms"]
KZ_ADAPTIVE_CONVERGED, KZ_ADAPTIVE_AT_CAP = 1, 2
KZ_TABLE_NODES, KZ_TABLE_NODES4, KZ_TABLE_TRIS, KZ_TABLE_SHADE, KZ_TABLE_CDF, KZ_TABLE_LIGHTS, KZ_TABLE_IL_TRIS, KZ_TABLE_PARAMS, KZ_TABLE_BSDFS, KZ_TABLE_EM_TRIS = range(10)
# exported by DEVELOPMENT builds of the library only (-DKZ_EXPERIMENTS): the hooks that are process-global state. The product library must NOT export them.
DEV_ONLY_EXPORTS = ["kz_debug_fail_alloc", "kz_debug_fail_device", "kz_debug_grow_delay", "kz_debug_trace", "kz_debug_alias_devices", "kz_debug_rr_ahead", "kz_debug_shadow_order", "kz_debug_compact_late"]

_HERE = os.path.dirname(os.path.abspath(__file__))
# KZ_LIB_PATH: a development build of the library (scripts/build_variant.sh) instead of the in-tree one; probes only
LIB_PATH = os.environ.get("KZ_LIB_PATH") or os.path.join(_HERE, "csrc", "libkazen_mi355x.so")
DEV_LIB_PATH = os.path.join(_HERE, "csrc", "variants", "experiments", "libkazen_mi355x.so")
_libs = {}


class KzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("kazen_mi355x error %d: %s" % (code, msg))
        self.code = code


def load_dev_library():
    """The development variant of the library (-DKZ_EXPERIMENTS: the same sources plus the hooks that are process-global state - kz_debug_fail_alloc /
    fail_device / grow_delay / trace / alias_devices / rr_ahead / shadow_order / compact_late). Only tests load it; a second copy of the library in one process is a separate world
    (its own device pools, its own replicas)."""
    return load_library(DEV_LIB_PATH)


def load_library(path=None):
    """Load the HIP extension. No fallback: a missing build is an error."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the product path has no CPU fallback)" % path)
    lib = C.CDLL(path)
    lib.kz_last_error.restype = C.c_char_p
    lib.kz_scene_create.argtypes = [C.POINTER(KzSceneDesc), C.POINTER(C.c_void_p)]
    lib.kz_scene_destroy.argtypes = [C.c_void_p]
    lib.kz_scene_destroy.restype = None
    lib.kz_scene_bvh_info.argtypes = [C.c_void_p, C.POINTER(KzBvhInfo)]
    lib.kz_scene_sample_count.argtypes = [C.c_void_p, u32p]
    lib.kz_scene_upload.argtypes = [C.c_void_p, C.c_int]
    lib.kz_render.argtypes = [C.c_void_p, C.POINTER(KzRenderOpts)]
    lib.kz_film_download.argtypes = [C.c_void_p, f32p, C.c_size_t]
    lib.kz_film_clear.argtypes = [C.c_void_p, C.c_void_p]
    lib.kz_film_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.kz_film_to_rgb.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, f32p]
    lib.kz_trace_rays.argtypes = [C.c_void_p, C.c_uint32, f32p, f32p, f32p, f32p, C.POINTER(KzHit)]
    if hasattr(lib, "kz_trace_rays_wf"):      # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_trace_rays_wf.argtypes = [C.c_void_p, C.POINTER(KzTraceWfOpts), C.c_uint32, f32p, f32p, f32p, f32p, u32p, C.c_uint32, f32p,
                                         C.POINTER(KzTraceWfHit), f32p, C.POINTER(KzTraceWfInfo)]
    lib.kz_set_stats.argtypes = [C.c_void_p, C.c_int]
    lib.kz_get_stats.argtypes = [C.c_void_p, C.POINTER(KzStats), C.c_int]
    lib.kz_sync.argtypes = [C.c_void_p]
    lib.kz_last_kernel_ms.argtypes = [C.c_void_p, f32p]
    lib.kz_last_stage_ms.argtypes = [C.c_void_p, f32p]
    lib.kz_render_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), u32p, f32p]
    lib.kz_bsdf_query.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p]
    lib.kz_film_to_srgb8.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t]
    lib.kz_texture_query.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), f32p, f32p]
    if hasattr(lib, "kz_camera_rays"):        # absent only in a KZ_LIB_PATH development build of older sources (same-call A/B runs)
        lib.kz_camera_rays.argtypes = [C.c_void_p, C.c_uint32, f32p, f32p, f32p]
        lib.kz_light_query.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), f32p, f32p, f32p]
    lib.kz_scene_evict.argtypes = [C.c_void_p, C.c_int]
    lib.kz_scene_devices.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, u32p]
    lib.kz_render_tiles.argtypes = [C.c_void_p, C.POINTER(KzRenderOpts), C.POINTER(KzTile), C.c_uint32, C.c_int, f32p, C.c_size_t]
    lib.kz_render_multi.argtypes = [C.c_void_p, C.POINTER(KzRenderOpts), C.POINTER(C.c_int32), C.c_uint32, C.c_int32, f32p, C.c_size_t, f32p]
    lib.kz_deal_tiles.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(KzTile), C.c_uint32, u32p]
    lib.kz_film_merge.argtypes = [f32p, f32p, C.c_size_t]
    lib.kz_tiles_packed_floats.argtypes = [C.c_void_p, C.POINTER(KzTile), C.c_uint32, C.POINTER(C.c_size_t)]
    lib.kz_film_download_tiles.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzTile), C.c_uint32, f32p, C.c_size_t]
    lib.kz_film_merge_tiles.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(KzTile), C.c_uint32, f32p, C.c_size_t, C.c_int32]
    lib.kz_film_merge_rects.argtypes = [f32p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(KzTile), C.POINTER(f32p), C.c_uint32, C.c_int32]
    lib.kz_film_download_on.argtypes = [C.c_void_p, C.c_int, f32p, C.c_size_t]
    lib.kz_film_clear_on.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.kz_sync_on.argtypes = [C.c_void_p, C.c_int]
    lib.kz_last_pass_info.argtypes = [C.c_void_p, C.POINTER(KzPassInfo)]
    lib.kz_pass_mode_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(KzPassModeInfo)]
    lib.kz_device_mem_info.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.kz_device_trim.argtypes = [C.c_int]
    lib.kz_last_grow_note.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    for hook in DEV_ONLY_EXPORTS:                 # development builds only
        if hasattr(lib, hook):
            getattr(lib, hook).argtypes = [C.c_int, C.c_int] if hook == "kz_debug_fail_device" else [C.c_int]
            getattr(lib, hook).restype = None
    if hasattr(lib, "kz_plan_passes"):
        lib.kz_plan_passes.argtypes = [C.POINTER(KzPlanQuery), C.POINTER(KzPlanAnswer)]
        lib.kz_plan_schedule.argtypes = [C.POINTER(KzPlanQuery), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32, u32p]
    if hasattr(lib, "kz_plan_pass_mode"):         # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_plan_pass_mode.argtypes = [C.POINTER(KzPassModeQuery), C.POINTER(KzPassModeState), C.POINTER(KzPassModeAnswer)]
    lib.kz_kat_dpdf.argtypes = [C.c_uint32, f32p, f32p, f32p]
    if hasattr(lib, "kz_scene_set_vertices"):     # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_scene_set_camera.argtypes = [C.c_void_p, C.POINTER(KzCamera)]
        lib.kz_scene_set_vertices.argtypes = [C.c_void_p, C.POINTER(KzVertexUpdate), C.c_uint32]
        lib.kz_scene_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(lib, "kz_scene_set_transforms"):
        lib.kz_scene_set_bsdfs.argtypes = [C.c_void_p, C.POINTER(KzBsdfUpdate), C.c_uint32]
        lib.kz_scene_set_lights.argtypes = [C.c_void_p, C.POINTER(KzLightUpdate), C.c_uint32]
        lib.kz_scene_set_transforms.argtypes = [C.c_void_p, C.POINTER(KzTransformUpdate), C.c_uint32]
    if hasattr(lib, "kz_scene_set_aovs"):         # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_scene_set_aovs.argtypes = [C.c_void_p, C.c_uint32]
        lib.kz_scene_aovs.argtypes = [C.c_void_p, u32p]
        lib.kz_aov_download.argtypes = [C.c_void_p, C.c_uint32, f32p, C.c_size_t]
        lib.kz_aov_download_on.argtypes = [C.c_void_p, C.c_int, C.c_uint32, f32p, C.c_size_t]
        lib.kz_aov_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        lib.kz_aov_samples.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), u32p, f32p]
    if hasattr(lib, "kz_denoise"):                # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_denoise.argtypes = [C.c_void_p, C.POINTER(KzDenoiseOpts)]
        lib.kz_denoise_on.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzDenoiseOpts)]
        lib.kz_denoise_download.argtypes = [C.c_void_p, C.c_int, f32p, C.c_size_t]
        lib.kz_denoise_to_srgb8.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.c_size_t]
        lib.kz_denoise_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        lib.kz_denoise_release.argtypes = [C.c_void_p, C.c_int]
        lib.kz_denoise_films.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, f32p, f32p, C.POINTER(KzDenoiseOpts), f32p]
    if hasattr(lib, "kz_denoise_variance"):       # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_scene_set_variance.argtypes = [C.c_void_p, C.c_int32]
        lib.kz_scene_variance.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        lib.kz_variance_download.argtypes = [C.c_void_p, C.c_int, f32p, C.c_size_t]
        lib.kz_variance_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), u32p]
        lib.kz_denoise_variance.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts)]
        lib.kz_denoise_variance_films.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, f32p, f32p, f32p, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts), f32p, f32p]
    if hasattr(lib, "kz_denoise_temporal"):       # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_temporal_view.argtypes = [C.POINTER(KzCamera), C.POINTER(KzTemporalView)]
        lib.kz_denoise_temporal.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts), C.POINTER(KzTemporalOpts)]
        lib.kz_temporal_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), u32p]
        lib.kz_temporal_reset.argtypes = [C.c_void_p, C.c_int]
        lib.kz_temporal_download.argtypes = [C.c_void_p, C.c_int, f32p, C.c_size_t]
        lib.kz_denoise_temporal_films.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, f32p, f32p, f32p, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts),
                                                  C.POINTER(KzTemporalOpts), C.POINTER(KzTemporalView), C.POINTER(KzTemporalView), f32p, f32p, f32p, f32p]
    if hasattr(lib, "kz_denoise_motion"):         # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_motion_rows.argtypes = [f32p, f32p, C.c_uint32, C.POINTER(KzMotionRow)]
        lib.kz_motion_ids.argtypes = [C.c_void_p, C.c_int, u32p, C.c_size_t]
        lib.kz_denoise_motion.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts), C.POINTER(KzTemporalOpts)]
        lib.kz_denoise_motion_films.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, f32p, f32p, f32p, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts),
                                                C.POINTER(KzTemporalOpts), C.POINTER(KzTemporalView), C.POINTER(KzTemporalView), f32p, u32p, C.POINTER(KzMotionRow), C.c_uint32,
                                                f32p, f32p, f32p]
        lib.kz_motion_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), u32p]
    if hasattr(lib, "kz_denoise_responsive"):     # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_denoise_responsive.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts), C.POINTER(KzTemporalOpts), C.POINTER(KzResponsiveOpts)]
        lib.kz_denoise_responsive_films.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, f32p, f32p, f32p, C.POINTER(KzDenoiseOpts), C.POINTER(KzVarianceOpts),
                                                    C.POINTER(KzTemporalOpts), C.POINTER(KzTemporalView), C.POINTER(KzTemporalView), f32p, u32p, C.POINTER(KzMotionRow), C.c_uint32,
                                                    f32p, f32p, f32p, C.POINTER(KzResponsiveOpts), f32p, f32p]
        lib.kz_responsive_download.argtypes = [C.c_void_p, C.c_int, f32p, C.c_size_t]
        lib.kz_responsive_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    if hasattr(lib, "kz_scene_set_mattes"):       # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_scene_set_mattes.argtypes = [C.c_void_p, C.c_uint32]
        lib.kz_scene_mattes.argtypes = [C.c_void_p, u32p]
        lib.kz_matte_download.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(KzMatteTexel), C.c_size_t]
        lib.kz_matte_download_on.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.POINTER(KzMatteTexel), C.c_size_t]
        lib.kz_matte_layer.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, f32p, C.c_size_t]
        lib.kz_matte_top.argtypes = [C.c_void_p, C.c_int, C.c_uint32, u32p, C.c_size_t]
        lib.kz_matte_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        lib.kz_matte_accumulate_items.argtypes = [C.c_void_p, C.c_int, u32p, C.c_uint32, C.c_uint32, u32p, C.POINTER(KzMatteTexel), C.c_uint32]
    if hasattr(lib, "kz_render_adaptive"):        # (absent only in a KZ_LIB_PATH development build of older sources)
        lib.kz_render_adaptive.argtypes = [C.c_void_p, C.POINTER(KzRenderOpts), C.POINTER(KzAdaptiveOpts), C.POINTER(KzAdaptiveInfo)]
        lib.kz_adaptive_blocks.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzAdaptiveBlock), C.c_size_t]
        lib.kz_adaptive_counts.argtypes = [C.c_void_p, C.c_int, u32p, C.c_size_t]
        lib.kz_adaptive_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(KzAdaptiveInfo)]
        lib.kz_adaptive_stage_ms.argtypes = [C.c_void_p, C.c_int, f32p]
        lib.kz_adaptive_classify_films.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, f32p, f32p, u32p, C.POINTER(KzAdaptiveOpts), C.POINTER(KzAdaptiveBlock)]
        lib.kz_adaptive_schedule.argtypes = [C.POINTER(KzAdaptiveOpts), C.c_uint32, u32p, C.c_uint32, u32p]
        lib.kz_adaptive_tiles.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(KzTile), C.c_uint32, u32p]
    lib.kz_kat_pow4.argtypes = [C.c_int32, C.POINTER(C.c_int32)]
    if hasattr(lib, "kz_kat_math"):
        lib.kz_kat_math.argtypes = [C.c_int, C.c_int, C.c_uint32, f32p, f32p, f32p]
    if hasattr(lib, "kz_kat_fresnel"):
        lib.kz_kat_fresnel.argtypes = [C.c_int, C.c_uint32, C.c_int, f32p, f32p, f32p, f32p]
    if hasattr(lib, "kz_kat_permute"):
        lib.kz_kat_permute.argtypes = [C.c_int, C.c_uint32, u32p, u32p, u32p, u32p]
    if hasattr(lib, "kz_kat_exact_math"):
        lib.kz_kat_exact_math.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    _libs[path] = lib
    return lib


def check(lib, rc):
    if rc != KZ_OK:
        msg = lib.kz_last_error()
        raise KzError(rc, msg.decode() if msg else "")

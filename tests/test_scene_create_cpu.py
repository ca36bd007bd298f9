"""No-GPU characterisation of kz_scene_create's refusals (kz_host.cpp): every case starts from the 16 x 16 Cornell box's KzSceneDesc with one field broken
(or two, for the cases that pin WHICH refusal a doubly wrong description gets) and holds the return code, the whole kz_last_error() text and a null *out.

Not covered - each needs an input no test should build, or cannot be reached through the checks in front of it:
  "%zu triangles (limit 2^28)" and the builder's "more than 2^28 triangle references"      (2^28 triangles)
  "scene too large: %zu BVH4 packets (limit 2^26 = 4 GB of packets)"                         (2^26 packets)
  "texture graphs flatten to more than 65536 operations", "more than 64 GB of texels"        (65536 texture ops, 64 GB of rasters)
  "pmj02bn table entry %d rounds to 1.0f ..."                                                 (a 2.6 MB table with one entry rounded up)
  "BVH build: BVH deeper than the traversal stack", "BVH4 collapse failed"                    (the builder caps its depth: test_abi_cpu.py's adversarial input stays inside)
  "filter radius %g needs too many taps"                                                      (a radius the (0, 4] check lets through needs nine taps at most)
  "background image index %d out of range", "background texture: filter %d"                  (every texture is flattened first, and the texture's own refusal
                                                                                               answers: test_two_faults holds that)
"""
import ctypes as C

import numpy as np
import pytest

INVALID, UNSUPPORTED = 1, 2
BSDF_TYPES = "diffuse, kazenstandard, mirror, dielectric, ggx, roughconductor, roughplastic, roughdielectric, normalmap"
ALPHA = "(0 or 1, and only roughconductor / roughplastic / roughdielectric rows have a resolved alpha)"
NESTED = "bsdf 0: normalmap needs a nested BSDF row that is not itself a normalmap (got %d)"


def _base(kz):
    """(KzSceneDesc of the small Cornell box: 8 meshes, 8 BSDF rows, 1 light, no textures; what keeps its memory alive)"""
    s = kz.scenes.cornell_box(16, 16, 1)
    return s.to_c(), [s]


def _textures(kz, d, keep, rows, images=()):
    """rows: dicts of KzTexture fields (child defaults to no children); images: (pixels, width, height, channels, format)"""
    a = kz.abi
    ct = (a.KzTexture * max(1, len(rows)))()
    for k, r in zip(ct, rows):
        k.child[:] = r.pop("child", (-1, -1, -1))
        for name, v in r.items():
            setattr(k, name, v)
    ci = (a.KzImage * max(1, len(images)))()
    for k, (px, w, h, ch, fmt) in zip(ci, images):
        k.pixels = px.ctypes.data if px is not None else None
        k.width, k.height, k.channels, k.format = w, h, ch, fmt
    d.textures, d.nTextures, d.images, d.nImages = ct, len(rows), ci, len(images)
    keep += [ct, ci, images]


def _set(path, value):
    """a case that sets one field: "camera.rfilter.radius", "meshes[0].bsdf", ..."""
    def mutate(kz, d, keep):
        obj, parts = d, path.split(".")
        for p in parts[:-1]:
            obj = getattr(obj, p[:p.index("[")])[int(p[p.index("[") + 1:-1])] if "[" in p else getattr(obj, p)
        setattr(obj, parts[-1], value)
    return mutate


def _both(*ms):
    def mutate(kz, d, keep):
        for m in ms:
            m(kz, d, keep)
    return mutate


def _normalmap(normalTex, nested, integrator=0):
    def mutate(kz, d, keep):
        _textures(kz, d, keep, [dict(type=kz.abi.KZ_TEX_CONSTANT)])
        d.bsdfs[0].type, d.bsdfs[0].normalTex, d.bsdfs[0].nested, d.integrator.type = kz.abi.KZ_BSDF_NORMALMAP, normalTex, nested, integrator
    return mutate


def _tex(rows, images=()):
    return lambda kz, d, keep: _textures(kz, d, keep, [dict(r) for r in rows], images)


def _stratified(res):
    return _both(_set("sampler.type", 2), _set("sampler.resolution", res))


def _face(mesh, value):
    def mutate(kz, d, keep):
        d.meshes[mesh].F[0] = value          # (the description's own array: every case flattens a fresh one)
    return mutate


def _background(texture):
    return _both(_set("background.present", 1), _set("background.texture", texture))


IMG = np.zeros((8, 8, 3), np.uint8)
IMAGE_TEX = dict(type=1, image=0, filter=0)
BLEND3 = [dict(type=3, child=(-1, -1, i + 1)) for i in range(3)] + [dict(type=3)]      # 2 operands held per level, 3 at the bottom: 9

ONE_FAULT = [
    ("abi", _set("abiVersion", 5), INVALID, "ABI version 5, library is 6"),
    ("camera_type", _set("camera.type", 99), UNSUPPORTED, 'camera type 99 is not supported ("perspective", "thinlens")'),
    ("integrator_type", _set("integrator.type", 99), UNSUPPORTED, 'integrator type 99 is not on the hot path ("path_mis", "normals", "ao", "path_mats")'),
    ("sampler_type", _set("sampler.type", 99), UNSUPPORTED, 'sampler type 99 is not supported ("independent", "pmj02bn", "stratified", "correlated")'),
    ("sampler_type_negative", _set("sampler.type", -1), UNSUPPORTED, 'sampler type -1 is not supported ("independent", "pmj02bn", "stratified", "correlated")'),
    ("stratified_resolution_0", _stratified(0), INVALID, "stratified resolution 0"),
    ("stratified_resolution_257", _stratified(257), INVALID, "stratified resolution 257"),
    ("sample_count_65537", _set("sampler.sampleCount", 65537), UNSUPPORTED, "sampleCount 65537 (limit 65536)"),
    ("rfilter_type", _set("camera.rfilter.type", 4), UNSUPPORTED, "rfilter type 4"),
    ("rfilter_type_negative", _set("camera.rfilter.type", -1), UNSUPPORTED, "rfilter type -1"),
    ("width_0", _set("camera.width", 0), INVALID, "image size 0x16"),
    ("height_65536", _set("camera.height", 65536), INVALID, "image size 16x65536"),
    ("sample_count_0", _set("sampler.sampleCount", 0), INVALID, "sampleCount is 0"),
    ("radius_0", _set("camera.rfilter.radius", 0.0), UNSUPPORTED, "filter radius 0 (supported: (0, 4])"),
    ("radius_4_5", _set("camera.rfilter.radius", 4.5), UNSUPPORTED, "filter radius 4.5 (supported: (0, 4])"),
    ("null_meshes", _set("meshes", None), INVALID, "null table with non-zero count"),
    ("null_bsdfs", _set("bsdfs", None), INVALID, "null table with non-zero count"),
    ("null_lights", _set("lights", None), INVALID, "null table with non-zero count"),
    ("null_textures", _both(_set("textures", None), _set("nTextures", 1)), INVALID, "null texture/image table with non-zero count"),
    ("null_images", _both(_set("images", None), _set("nImages", 1)), INVALID, "null texture/image table with non-zero count"),
    # kzCheckBsdfs through create
    ("bsdf_type", _set("bsdfs[0].type", 99), UNSUPPORTED, "bsdf 0 has type 99 (supported: %s)" % BSDF_TYPES),
    ("bsdf_texture_id", _set("bsdfs[0].albedoTex", 1), INVALID, "bsdf 0: texture id 1 out of range (0 = constant, 1..0)"),
    ("bsdf_texture_id_negative", _set("bsdfs[3].metallicTex", -1), INVALID, "bsdf 3: texture id -1 out of range (0 = constant, 1..0)"),
    ("bsdf_texture_unread", _both(_tex([dict(type=0)]), _set("bsdfs[0].roughnessTex", 1)), INVALID,
     "bsdf 0 (type 0): a texture id is set on a parameter this model does not read through a texture"),
    ("bsdf_alpha_resolved_2", _set("bsdfs[0].alphaResolved", 2), INVALID, "bsdf 0 (type 0): alphaResolved = 2 " + ALPHA),
    ("bsdf_alpha_resolved_diffuse", _set("bsdfs[0].alphaResolved", 1), INVALID, "bsdf 0 (type 0): alphaResolved = 1 " + ALPHA),
    ("normalmap_path_mats", _normalmap(1, 1, integrator=3), UNSUPPORTED,
     "bsdf 0 is a normalmap: path_mats does not support normal maps (its BSDF record carries no intersection frame)"),
    ("normalmap_no_texture", _normalmap(0, 1), INVALID, "bsdf 0: normalmap without a normal texture"),
    ("normalmap_nested_negative", _normalmap(1, -1), INVALID, NESTED % -1),
    ("normalmap_nested_past_end", _normalmap(1, 8), INVALID, NESTED % 8),
    ("normalmap_nested_normalmap", _normalmap(1, 0), INVALID, NESTED % 0),
    # images and texture graphs
    ("image_width_0", _tex([], [(IMG, 0, 8, 3, 0)]), INVALID, "image 0: 0x8x3 format 0"),
    ("image_format", _tex([], [(IMG, 8, 8, 3, 0), (IMG, 8, 8, 3, 2)]), INVALID, "image 1: 8x8x3 format 2"),
    ("image_null_pixels", _tex([], [(None, 8, 8, 3, 0)]), INVALID, "image 0: 8x8x3 format 0"),
    ("image_channels_17", _tex([], [(IMG, 8, 8, 17, 0)]), INVALID, "image 0: 8x8x17 format 0"),
    ("texture_cycle", _tex([dict(type=2, child=(0, -1, -1))]), UNSUPPORTED, "texture graph is cyclic or deeper than 32 levels"),
    ("texture_child", _tex([dict(type=2, child=(5, -1, -1))]), INVALID, "texture 0: child 5 out of range"),
    ("texture_image_index", _tex([dict(type=0), dict(type=1, image=3)]), INVALID, "texture 1: image index 3 out of range"),
    ("texture_image_index_negative", _tex([dict(type=1, image=-1)], [(IMG, 8, 8, 3, 0)]), INVALID, "texture 0: image index -1 out of range"),
    ("texture_filter", _tex([dict(type=1, image=0, filter=2)], [(IMG, 8, 8, 3, 0)]), INVALID, "texture 0: filter 2 (KZ_TEXFILTER_BILINEAR or KZ_TEXFILTER_BICUBIC)"),
    ("texture_blend_mode", _tex([dict(type=3, blendMode=3)]), INVALID, "texture 0: blend mode 3"),
    ("texture_type", _tex([dict(type=9)]), UNSUPPORTED, "texture 0 has type 9 (supported: constanttexture, imagetexture, colorramp, blend)"),
    ("texture_stack", _tex(BLEND3), UNSUPPORTED, "texture 0 needs an operand stack of 9 (limit 8)"),
    # meshes
    ("mesh_no_V", _set("meshes[0].V", None), INVALID, "mesh 0 has no V/F"),
    ("mesh_no_F", _set("meshes[3].F", None), INVALID, "mesh 3 has no V/F"),
    ("mesh_bsdf_past_end", _set("meshes[0].bsdf", 8), INVALID, "mesh 0: bsdf/light index out of range"),
    ("mesh_bsdf_minus_2", _set("meshes[1].bsdf", -2), INVALID, "mesh 1: bsdf/light index out of range"),
    ("mesh_light_past_end", _set("meshes[2].light", 1), INVALID, "mesh 2: bsdf/light index out of range"),
    ("mesh_light_minus_2", _set("meshes[7].light", -2), INVALID, "mesh 7: bsdf/light index out of range"),
    ("vertex_index", _face(0, 999), INVALID, "mesh 0 face 0: vertex index 999 >= 4"),
    ("vertex_index_is_nV", _face(7, 4), INVALID, "mesh 7 face 0: vertex index 4 >= 4"),
    # camera, background, sampler tables
    ("singular_projection", _set("camera.nearClip", 0.0), INVALID, "singular projection (fov 39, clip 0..100)"),
    ("background_texture", _background(5), INVALID, "background texture id 5 out of range"),
    ("background_texture_negative", _background(-1), INVALID, "background texture id -1 out of range"),
    ("pmj02bn_no_tables", _set("sampler.type", 1), INVALID, "pmj02bn sampler without its tables"),
]

# a description wrong in two ways gets the refusal of the check that comes first
TWO_FAULTS = [
    ("abi_before_camera", _both(_set("camera.type", 99), _set("abiVersion", 5)), INVALID, "ABI version 5, library is 6"),
    ("rfilter_type_before_sample_count_0", _both(_set("sampler.sampleCount", 0), _set("camera.rfilter.type", 9)), UNSUPPORTED, "rfilter type 9"),
    ("image_size_before_sample_count_0", _both(_set("sampler.sampleCount", 0), _set("camera.width", 0)), INVALID, "image size 0x16"),
    ("sample_count_65537_before_image_size", _both(_set("camera.width", 0), _set("sampler.sampleCount", 65537)), UNSUPPORTED, "sampleCount 65537 (limit 65536)"),
    ("bsdf_before_image", _both(_tex([], [(IMG, 0, 8, 3, 0)]), _set("bsdfs[2].type", 99)), UNSUPPORTED, "bsdf 2 has type 99 (supported: %s)" % BSDF_TYPES),
    ("image_before_texture", _tex([dict(type=9)], [(IMG, 8, 8, 0, 0)]), INVALID, "image 0: 8x8x0 format 0"),
    ("texture_before_mesh", _both(_tex([dict(type=9)]), _set("meshes[0].V", None)), UNSUPPORTED,
     "texture 0 has type 9 (supported: constanttexture, imagetexture, colorramp, blend)"),
    ("mesh_before_pmj02bn_tables", _both(_set("sampler.type", 1), _set("meshes[0].V", None)), INVALID, "mesh 0 has no V/F"),
    ("first_mesh_before_second", _both(_set("meshes[1].V", None), _face(0, 999)), INVALID, "mesh 0 face 0: vertex index 999 >= 4"),
    ("vertex_index_before_background", _both(_background(5), _face(0, 999)), INVALID, "mesh 0 face 0: vertex index 999 >= 4"),
    ("projection_before_background", _both(_background(5), _set("camera.nearClip", 0.0)), INVALID, "singular projection (fov 39, clip 0..100)"),
    ("background_before_pmj02bn_tables", _both(_set("sampler.type", 1), _background(5)), INVALID, "background texture id 5 out of range"),
    # the background's image texture is refused as the texture it is, never as the background
    ("texture_before_background_image", _both(_tex([dict(type=1, image=3)]), _background(1)), INVALID, "texture 0: image index 3 out of range"),
    ("texture_before_background_filter", _both(_tex([dict(type=1, image=0, filter=2)], [(IMG, 8, 8, 3, 0)]), _background(1)), INVALID,
     "texture 0: filter 2 (KZ_TEXFILTER_BILINEAR or KZ_TEXFILTER_BICUBIC)"),
]


def _refused(kz, lib, mutate, code, text):
    d, keep = _base(kz)
    mutate(kz, d, keep)
    h = C.c_void_p(0xDEAD)                       # (never dereferenced: create writes null over it before anything can fail)
    assert lib.kz_scene_create(C.byref(d), C.byref(h)) == code
    assert lib.kz_last_error().decode() == text
    assert h.value is None


@pytest.mark.parametrize("mutate,code,text", [c[1:] for c in ONE_FAULT], ids=[c[0] for c in ONE_FAULT])
def test_one_fault(kz, mutate, code, text):
    _refused(kz, kz.abi.load_library(), mutate, code, text)


@pytest.mark.parametrize("mutate,code,text", [c[1:] for c in TWO_FAULTS], ids=[c[0] for c in TWO_FAULTS])
def test_two_faults(kz, mutate, code, text):
    _refused(kz, kz.abi.load_library(), mutate, code, text)


def test_null_arguments(kz):
    lib = kz.abi.load_library()
    d, keep = _base(kz)
    h = C.c_void_p()
    for args in ((None, C.byref(h)), (C.byref(d), None), (None, None)):
        assert lib.kz_scene_create(*args) == INVALID
        assert lib.kz_last_error().decode() == "kz_scene_create: null argument"
        assert h.value is None


def test_a_refusal_leaves_nothing_behind(kz):
    """The valid description is created after every refusal and comes out as it did before the first one, table by table."""
    lib = kz.abi.load_library()

    def tables():
        sc = kz.Scene(kz.scenes.cornell_box(16, 16, 1), lib=lib)
        out = [sc.table(t).tobytes() for t in range(10)]
        sc.close()
        return out
    want = tables()
    assert all(len(t) for t in want[:8])
    for name, mutate, code, text in ONE_FAULT + TWO_FAULTS:
        _refused(kz, lib, mutate, code, text)
        assert tables() == want, name

"""The test-only CPU references (tests/cpu_ref/*.cpp) the GPU tests compare against, built and called one way: a table of the eight libraries, lib() that compiles
one and declares its entries, the scene of a reference, and the callers of the references' entries. A support module beside the tests, like sample_corners.py:
imported by the tests and by scripts/*_quality.py, never collected."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INTEGRATOR_TAGS = {"path_mis": 0, "normals": 1, "ao": 2, "path_mats": 3}

_i, _u, _z, _p = C.c_int, C.c_uint32, C.c_size_t, C.c_void_p
_f32p, _u32p, _i32p, _ip = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_int)
_SAMPLES = [_p, _i, _u, _i32p, _u32p]                               # scene, integrator tag, n, pixels, sample indices - then the output
_CANONICAL = [_p, _i, _u, _u, _i, _i, _f32p]                        # scene, integrator tag, s0, s1, threads, grid, film
_FILMS = [_i, _i, _i] + [_f32p] * 5                                 # w, h, border, film, moment, albedo, normal, depth
_HISTORY = _FILMS + [_p] * 5 + [_f32p]                              # ... KzDenoiseOpts, KzVarianceOpts, KzTemporalOpts, current, previous, history
_MOTION = _HISTORY + [_u32p, _p, _u]                                # ... ids, rows, nRows
_OUT = [_f32p] * 3                                                  # film, history, v_last

# name -> (source under tests/cpu_ref, -pthread?, the name whose entries it inherits - its source #includes that one's -, {entry it adds: (argtypes, restype)}).
# "oracle" is oracle/kz_oracle.cpp itself: no library of its own, the entries every source that includes it inherits. None for argtypes leaves them undeclared.
REFS = {
    "oracle": (None, None, None, {"kzo_last_error": (None, C.c_char_p), "kzo_scene_create": (["KzSceneDesc*", _i, C.POINTER(_p)], _i), "kzo_scene_destroy": ([_p], None),
                                  "kzo_film_dims": ([_p, _ip, _ip, _ip], _i)}),
    "aov": ("kz_aov_ref.cpp", True, "oracle", {"kza_samples": (_SAMPLES + [_f32p], None), "kza_render_canonical": ([_p, _i, _u, _u, _u, _i, _i, _f32p], _i)}),
    "integrators": ("kz_integrators_ref.cpp", True, "oracle", {"kzi_render_samples": (_SAMPLES + [_f32p], None), "kzi_render_canonical": (_CANONICAL, _i),
                                                               "kzi_mats_depth": ([_p, C.c_int32, C.c_int32, _u], _i)}),
    "matte": ("kz_matte_ref.cpp", True, "oracle", {"kzm_samples": (_SAMPLES + [_u32p], None), "kzm_table": ([_p, _i, _u, _u, _u, _i, _i, _i, _i, _p], _i),
                                                   "kzm_accumulate": ([_u32p, _u, _u, _p], None), "kzm_rank": ([_p, _z, _p], None), "kzm_layer": ([_p, _z, _u, _f32p], None),
                                                   "kzm_top": ([_p, _z, _u32p], None)}),
    "denoise": ("kz_denoise_ref.cpp", False, None, {"kzd_denoise": ([_i, _i, _i] + [_f32p] * 4 + [_p, _f32p], _i)}),
    "variance": ("kz_variance_ref.cpp", True, "integrators", {"kzv_render_canonical": (_CANONICAL, _i), "kzv_denoise": (_FILMS + [_p, _p, _f32p, _f32p], _i)}),
    "temporal": ("kz_temporal_ref.cpp", True, "variance", {"kzt_denoise": (_HISTORY + _OUT, _i)}),
    "motion": ("kz_motion_ref.cpp", True, "temporal", {"kzm_denoise": (_MOTION + _OUT, _i), "kzm_ids": ([_p, _i, _u32p], None)}),
    "responsive": ("kz_responsive_ref.cpp", True, "motion", {"kzr_denoise": (_MOTION + _OUT + [_p, _f32p, _f32p], _i)}),
}
_libs = {}


def lib(name, tmpdir):
    """The reference library `name`, compiled with the oracle's flags into `tmpdir` once per process, its own entries and those it inherits declared."""
    if name not in _libs:
        import oracle
        source, pthread = REFS[name][:2]
        out = os.path.join(str(tmpdir), "libkz_%s_ref.so" % name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"] + (["-pthread"] if pthread else []) +
                              ["-I" + os.path.join(ROOT, "include"), "-o", out, os.path.join(HERE, "cpu_ref", source)])
        L = C.CDLL(out)
        link = name
        while link is not None:
            _, _, link, entries = REFS[link]
            for fn, (argtypes, restype) in entries.items():
                if argtypes is not None:
                    getattr(L, fn).argtypes = [C.POINTER(oracle.abi.KzSceneDesc) if t == "KzSceneDesc*" else t for t in argtypes]
                getattr(L, fn).restype = restype
        _libs[name] = L
    return _libs[name]


# ---------------------------------------------------------------- the scene of a reference
class ReferenceScene:
    """A scene of a CPU reference: created through the oracle's kzo_scene_create with the path_mis tag, as the oracle demands; the integrator named in the
    description (or here) is kept as `tag` and handed to the entries, where it picks the Li and decides whether a first hit on an invisible light is walked through."""

    def __init__(self, L, desc, integrator=None):
        import oracle
        self.L, self.abi = L, oracle.abi
        self.integ = desc.integrator["type"] if integrator is None else integrator
        d = copy.copy(desc)
        d.integrator = dict(desc.integrator, type="path_mis")
        self._c = d.to_c()
        h = C.c_void_p()
        rc = L.kzo_scene_create(C.byref(self._c), 0, C.byref(h))
        if rc != 0:
            raise self.abi.KzError(rc, L.kzo_last_error().decode())
        self.h = h
        w, hh, b = C.c_int(), C.c_int(), C.c_int()
        L.kzo_film_dims(self.h, C.byref(w), C.byref(hh), C.byref(b))
        self.width, self.height, self.border = w.value, hh.value, b.value
        self.tag = INTEGRATOR_TAGS[self.integ]

    def __del__(self):
        if getattr(self, "h", None):
            self.L.kzo_scene_destroy(self.h)

    def _samples(self, fn, pxy, idx, columns, dtype):
        pxy = np.ascontiguousarray(pxy, np.int32)
        idx = np.ascontiguousarray(idx, np.uint32)
        out = np.zeros((idx.shape[0], columns), dtype)
        fn(self.h, self.tag, idx.shape[0], pxy.ctypes.data_as(_i32p), idx.ctypes.data_as(_u32p), out.ctypes.data_as(_f32p if dtype is np.float32 else _u32p))
        return out

    def _film(self, fn, *args):
        film = np.zeros((self.height + 2 * self.border, self.width + 2 * self.border, 4), np.float32)
        assert fn(self.h, self.tag, *args, film.ctypes.data_as(_f32p)) == 0
        return film


class AovRef(ReferenceScene):
    """lib("aov"): the feature films' samples and canonical films."""

    def samples(self, pxy, idx):
        return self._samples(self.L.kza_samples, pxy, idx, 10, np.float32)

    def film(self, aov, s0=0, s1=0, threads=16, grid=64):
        return self._film(self.L.kza_render_canonical, {"albedo": 1, "normal": 2, "depth": 4}[aov], s0, s1, threads, grid)


class RefScene(ReferenceScene):
    """lib("integrators"): rendered with the integrator named."""

    def render_samples(self, pxy, idx):
        return self._samples(self.L.kzi_render_samples, pxy, idx, 5, np.float32)

    def render_canonical(self, s0=0, s1=0, threads=16, grid=64):
        return self._film(self.L.kzi_render_canonical, s0, s1, threads, grid)

    def mats_depth(self, px, py, idx):
        return int(self.L.kzi_mats_depth(self.h, px, py, idx))


class MomentRef(ReferenceScene):
    """lib("variance") and the libraries that inherit it: the canonical second-moment film and, from the same translation unit, the canonical picture."""

    def moment_film(self, s0=0, s1=0, threads=16, grid=64):
        return self._film(self.L.kzv_render_canonical, s0, s1, threads, grid)

    def film(self, s0=0, s1=0, threads=16, grid=64):
        return self._film(self.L.kzi_render_canonical, s0, s1, threads, grid)


class MatteRef(ReferenceScene):
    """lib("matte"): the matte entry points; `dtype` is the record's (kz.abi.MATTE_DTYPE)."""

    def __init__(self, L, desc, dtype, integrator=None):
        super().__init__(L, desc, integrator)
        self.dtype = dtype

    def samples(self, pxy, idx):
        """(n, 3) uint32: mesh | bsdf row | hit."""
        return self._samples(self.L.kzm_samples, pxy, idx, 3, np.uint32)

    def table(self, key, s0, s1, start=None, rect=None):
        """The (h, w) table of `key` after the samples [s0, s1) of `rect` (x0, y0, w, h; None: the frame) on top of `start` (None: zeros). Unranked."""
        t = np.zeros((self.height, self.width), self.dtype) if start is None else np.ascontiguousarray(start, self.dtype).copy()
        x0, y0, w, h = rect or (0, 0, self.width, self.height)
        assert self.L.kzm_table(self.h, self.tag, {"mesh": 1, "bsdf": 2}[key], s0, s1, x0, y0, w, h, t.ctypes.data) == 0
        return t


_moments = {}


def ref_moment(ref, key, desc, s0=0, s1=0):
    """The reference's second-moment film of a description, computed once per (key, sample range) and shared."""
    k = (key, s0, s1)
    if k not in _moments:
        _moments[k] = MomentRef(ref, desc).moment_film(s0, s1)
        _moments[k].setflags(write=False)
    return _moments[k]


def ref_ids(L, desc):
    """The reference's ids (h, w) of a description: the oracle's camera ray at every pixel centre, its closest hit and, for path_mis, its walk-through."""
    r = ReferenceScene(L, desc)
    ids = np.zeros((r.height, r.width), np.uint32)
    L.kzm_ids(r.h, r.tag, ids.ctypes.data_as(_u32p))
    return ids


# ---------------------------------------------------------------- the mattes' table functions
def ref_accumulate(L, dtype, keys, start=None):
    keys = np.ascontiguousarray(keys, np.uint32)
    t = np.zeros(keys.shape[0], dtype) if start is None else np.ascontiguousarray(start, dtype).copy()
    L.kzm_accumulate(keys.ctypes.data_as(_u32p), keys.shape[0], keys.shape[1], t.ctypes.data)
    return t


def ref_rank(L, t):
    t = np.ascontiguousarray(t)
    out = np.zeros_like(t)
    L.kzm_rank(t.ctypes.data, t.size, out.ctypes.data)
    return out


def ref_layer(L, t, id):
    t = np.ascontiguousarray(t)
    out = np.zeros(t.shape, np.float32)
    L.kzm_layer(t.ctypes.data, t.size, id, out.ctypes.data_as(_f32p))
    return out


def ref_top(L, t):
    t = np.ascontiguousarray(t)
    out = np.zeros(t.shape, np.uint32)
    L.kzm_top(t.ctypes.data, t.size, out.ctypes.data_as(_u32p))
    return out


# ---------------------------------------------------------------- the denoisers
def _ptr(a):
    return None if a is None else a.ctypes.data_as(_f32p)


def _films(film, guides, border):
    """(film, guides) as contiguous fp32 arrays (a guide may be None), an output film of NaNs, and the frame's (h, w)."""
    film = np.ascontiguousarray(film, np.float32)
    g = [None if a is None else np.ascontiguousarray(a, np.float32) for a in guides]
    return film, g, np.full(film.shape, np.nan, np.float32), (film.shape[0] - 2 * border, film.shape[1] - 2 * border)


def ref_denoise(L, kz, film, albedo=None, normal=None, depth=None, border=0, **opts):
    """The reference's film of four films (guides may be None); options as kz.denoise_opts takes them."""
    film, g, out, (h, w) = _films(film, (albedo, normal, depth), border)
    o = kz.denoise_opts(**opts)
    rc = L.kzd_denoise(w, h, border, _ptr(film), *[_ptr(a) for a in g], C.byref(o), _ptr(out))
    assert rc == 0, "the reference refused the options"
    return out


def ref_denoise_variance(L, kz, film, moment, albedo=None, normal=None, depth=None, border=0, samples=4, sigma_variance=0.0, **opts):
    """The reference's (film, v_last) of five films (guides may be None); options as kz.denoise_opts / kz.variance_opts take them."""
    film, g, out, (h, w) = _films(film, (moment, albedo, normal, depth), border)
    var = np.full((h, w), np.nan, np.float32)
    o, v = kz.denoise_opts(**opts), kz.variance_opts(sigma_variance, samples)
    rc = L.kzv_denoise(w, h, border, _ptr(film), *[_ptr(a) for a in g], C.byref(o), C.byref(v), _ptr(out), _ptr(var))
    assert rc == 0, "the reference refused the options"
    return out, var


def _history_call(kz, film, guides, border, samples, sigma_variance, current, previous, history, depth_tolerance, normal_tolerance, max_history, opts, ids=None,
                  rows=None, n_rows=None, motion=False):
    """What kzt_denoise, kzm_denoise and kzr_denoise share, as _history_films of render.py prepares it for the product: the arguments up to the outputs - the
    frame, the five films, the three option structs, the two views, the history as (h, w, 12), and for `motion` the ids as (h, w) and the row table - then the
    outputs (film, history (h, w, 12), v_last (h, w)), filled with NaN, and the frame's (h, w)."""
    film, g, out, (h, w) = _films(film, guides, border)
    history = None if history is None else np.ascontiguousarray(history, np.float32).reshape(h, w, 12)
    hist, var = np.full((h, w, 12), np.nan, np.float32), np.full((h, w), np.nan, np.float32)
    o, v, t = kz.denoise_opts(**opts), kz.variance_opts(sigma_variance, samples), kz.temporal_opts(depth_tolerance, normal_tolerance, max_history)
    args = [w, h, border, _ptr(film), *[_ptr(a) for a in g], C.byref(o), C.byref(v), C.byref(t), None if current is None else C.byref(current),
            None if previous is None else C.byref(previous), _ptr(history)]
    if motion:
        ids = np.ascontiguousarray(ids, np.uint32).reshape(h, w)
        args += [ids.ctypes.data_as(_u32p), C.byref(rows), getattr(rows, "n_rows", len(rows)) if n_rows is None else n_rows]
    return args + [_ptr(out), _ptr(hist), _ptr(var)], (out, hist, var), (h, w)


def ref_denoise_temporal(L, kz, film, moment, albedo=None, normal=None, depth=None, border=0, samples=4, sigma_variance=0.0, current=None, previous=None, history=None,
                         depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, **opts):
    """The reference's (film, history (h, w, 12), v_last) of five films (albedo / normal may be None), the two views and a history (None: none); options as
    kz.denoise_opts / kz.variance_opts / kz.temporal_opts take them."""
    args, outs, _ = _history_call(kz, film, (moment, albedo, normal, depth), border, samples, sigma_variance, current, previous, history, depth_tolerance, normal_tolerance,
                                  max_history, opts)
    assert L.kzt_denoise(*args) == 0, "the reference refused the options"
    return outs


def ref_denoise_motion(L, kz, film, moment, albedo=None, normal=None, depth=None, border=0, samples=4, sigma_variance=0.0, current=None, previous=None, history=None,
                       ids=None, rows=None, n_rows=None, depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, **opts):
    """The reference's (film, history (h, w, 12), v_last): ref_denoise_temporal's arguments plus ids (h, w) and rows (a KzMotionRow array as kz.motion_rows gives it)."""
    args, outs, _ = _history_call(kz, film, (moment, albedo, normal, depth), border, samples, sigma_variance, current, previous, history, depth_tolerance, normal_tolerance,
                                  max_history, opts, ids, rows, n_rows, motion=True)
    rc = L.kzm_denoise(*args)
    assert rc == 0, "the reference refused the call (%d)" % rc
    return outs


def ref_denoise_responsive(L, kz, film, moment, albedo=None, normal=None, depth=None, border=0, samples=4, sigma_variance=0.0, current=None, previous=None, history=None,
                           ids=None, rows=None, n_rows=None, depth_tolerance=0.0, normal_tolerance=0.0, max_history=0, fast=None, fast_history=0, clamp_sigma=0.0, radius=0,
                           clamp=True, **opts):
    """The reference's (film, history (h, w, 12), fast (h, w, 4), v_last): ref_denoise_motion's arguments plus the fast plane (None: absent) and responsive_opts'."""
    args, (out, hist, var), (h, w) = _history_call(kz, film, (moment, albedo, normal, depth), border, samples, sigma_variance, current, previous, history, depth_tolerance,
                                                    normal_tolerance, max_history, opts, ids, rows, n_rows, motion=True)
    fast = None if fast is None else np.ascontiguousarray(fast, np.float32).reshape(h, w, 4)
    fout = np.full((h, w, 4), np.nan, np.float32)
    r = kz.responsive_opts(fast_history, clamp_sigma, radius, clamp)
    rc = L.kzr_denoise(*args, C.byref(r), _ptr(fast), _ptr(fout))
    assert rc == 0, "the reference refused the call (%d)" % rc
    return out, hist, fout, var

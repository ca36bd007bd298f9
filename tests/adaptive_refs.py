"""The test-only CPU reference of adaptive sampling (tests/cpu_ref/kz_adaptive_ref.cpp), built with cpu_refs' compile line, the callers of its entries, and the
Python restatements of the two pure host functions (the round schedule and the tile list). A support module beside the tests, like cpu_refs.py: imported by the
adaptive tests and by scripts/adaptive_rates.py, never collected."""
import ctypes as C
import os
import subprocess

import numpy as np

import cpu_refs

_i, _u, _p = C.c_int, C.c_uint32, C.c_void_p
_f32p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
BLOCK_DTYPE = [("samples", "<u4"), ("noisy", "<u4"), ("valid", "<u4"), ("flags", "<u4")]
CONVERGED, AT_CAP = 1, 2

# the entries kz_adaptive_ref.cpp adds to those of "variance" (whose source it includes)
ENTRIES = {"kzad_render_counts": ([_p, _i, _i, _u32p, _i, _i, _f32p], _i),
           "kzad_classify": ([_i, _i, _i, _f32p, _f32p, _u32p, _p, _p], _i),
           "kzad_adaptive": ([_p, _i, _p, _i, _i, _f32p, _f32p, _p, _u32p, _u32p], _i)}
_lib = None


def lib(tmpdir):
    """The reference library, compiled as cpu_refs.lib compiles its own into `tmpdir` once per process; its entries and those it inherits declared."""
    global _lib
    if _lib is None:
        import oracle
        out = os.path.join(str(tmpdir), "libkz_adaptive_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(cpu_refs.ROOT, "include"), "-o", out,
                               os.path.join(cpu_refs.HERE, "cpu_ref", "kz_adaptive_ref.cpp")])
        L = C.CDLL(out)
        tables, link = [ENTRIES], "variance"
        while link is not None:
            tables.append(cpu_refs.REFS[link][3])
            link = cpu_refs.REFS[link][2]
        for entries in tables:
            for fn, (argtypes, restype) in entries.items():
                if argtypes is not None:
                    getattr(L, fn).argtypes = [C.POINTER(oracle.abi.KzSceneDesc) if t == "KzSceneDesc*" else t for t in argtypes]
                getattr(L, fn).restype = restype
        _lib = L
    return _lib


_aov_lib = None


def aov_lib(tmpdir):
    """tests/cpu_ref/kz_adaptive_aov_ref.cpp (kz_aov_ref.cpp + the feature films of a plane of per-pixel counts), compiled the same way."""
    global _aov_lib
    if _aov_lib is None:
        import oracle
        out = os.path.join(str(tmpdir), "libkz_adaptive_aov_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(cpu_refs.ROOT, "include"), "-o", out,
                               os.path.join(cpu_refs.HERE, "cpu_ref", "kz_adaptive_aov_ref.cpp")])
        L = C.CDLL(out)
        for entries in ({"kzada_render_counts": ([_p, _i, _u, _u32p, _i, _i, _f32p], _i)}, cpu_refs.REFS["oracle"][3]):
            for fn, (argtypes, restype) in entries.items():
                if argtypes is not None:
                    getattr(L, fn).argtypes = [C.POINTER(oracle.abi.KzSceneDesc) if t == "KzSceneDesc*" else t for t in argtypes]
                getattr(L, fn).restype = restype
        _aov_lib = L
    return _aov_lib


def ref_aov_counts(L, desc, aov, counts, threads=16, grid=64):
    """The canonical feature film `aov` ("albedo", "normal", "depth") of a frame whose pixel (x, y) holds the samples [0, counts[y, x]); L: aov_lib's."""
    r = cpu_refs.ReferenceScene(L, desc)
    counts = np.ascontiguousarray(counts, np.uint32)
    film = np.zeros((r.height + 2 * r.border, r.width + 2 * r.border, 4), np.float32)
    assert L.kzada_render_counts(r.h, r.tag, {"albedo": 1, "normal": 2, "depth": 4}[aov], counts.ctypes.data_as(_u32p), threads, grid, film.ctypes.data_as(_f32p)) == 0
    return film


class AdaptiveRef(cpu_refs.MomentRef):
    """A scene of the reference: MomentRef's canonical films, the films of a plane of per-pixel counts, and the whole adaptive call."""

    def film_counts(self, which, counts, threads=16, grid=64):
        """The canonical film (which = 0: the picture, 1: the second-moment film) of a frame whose pixel (x, y) holds the samples [0, counts[y, x])."""
        counts = np.ascontiguousarray(counts, np.uint32)
        assert counts.shape == (self.height, self.width)
        film = np.zeros((self.height + 2 * self.border, self.width + 2 * self.border, 4), np.float32)
        assert self.L.kzad_render_counts(self.h, self.tag, which, counts.ctypes.data_as(_u32p), threads, grid, film.ctypes.data_as(_f32p)) == 0
        return film

    def adaptive(self, opts, threads=16, grid=64):
        """kzad_adaptive with a KzAdaptiveOpts: (film, moment, records (1-D, BLOCK_DTYPE), counts (h, w), rounds)."""
        e = opts.block or 16
        film = np.zeros((self.height + 2 * self.border, self.width + 2 * self.border, 4), np.float32)
        moment = np.zeros_like(film)
        rec = np.zeros(((self.height + e - 1) // e) * ((self.width + e - 1) // e), BLOCK_DTYPE)
        counts, rounds = np.zeros((self.height, self.width), np.uint32), C.c_uint32()
        rc = self.L.kzad_adaptive(self.h, self.tag, C.byref(opts), threads, grid, film.ctypes.data_as(_f32p), moment.ctypes.data_as(_f32p), rec.ctypes.data,
                                  counts.ctypes.data_as(_u32p), C.byref(rounds))
        assert rc == 0, "the reference refused the options"
        return film, moment, rec, counts, int(rounds.value)


def ref_classify(L, film, moment, block_samples, opts, border=0):
    """kzad_classify on host films with a KzAdaptiveOpts: the records, 1-D of BLOCK_DTYPE."""
    film, moment = np.ascontiguousarray(film, np.float32), np.ascontiguousarray(moment, np.float32)
    h, w, e = film.shape[0] - 2 * border, film.shape[1] - 2 * border, opts.block or 16
    ns = np.ascontiguousarray(np.asarray(block_samples).ravel(), np.uint32)
    out = np.zeros(((h + e - 1) // e) * ((w + e - 1) // e), BLOCK_DTYPE)
    assert ns.size == out.size
    rc = L.kzad_classify(w, h, border, film.ctypes.data_as(_f32p), moment.ctypes.data_as(_f32p), ns.ctypes.data_as(_u32p), C.byref(opts), out.ctypes.data)
    assert rc == 0, "the reference refused the options"
    return out


# ---------------------------------------------------------------- Python restatements of the pure host functions
def py_schedule(scene_samples, min_samples=0, max_samples=0, step=0):
    """The header's schedule: n_0 = min(minSamples, maxSamples), then min(maxSamples, step ? n + step : 2 n) until maxSamples."""
    cap = max_samples or scene_samples
    n = min(min_samples or min(16, cap), cap)
    out = [n]
    while n != cap:
        n = min(cap, n + step if step else 2 * n)
        out.append(n)
    return out


def py_tiles(width, height, block, active):
    """The header's tile list: block rows top to bottom, every maximal horizontal run of active blocks one tile, edge blocks clipped."""
    nbx, nby = (width + block - 1) // block, (height + block - 1) // block
    active = np.asarray(active).reshape(nby, nbx)
    tiles = []
    for by in range(nby):
        bx = 0
        while bx < nbx:
            if not active[by, bx]:
                bx += 1
                continue
            end = bx
            while end < nbx and active[by, end]:
                end += 1
            x0, y0 = bx * block, by * block
            tiles.append((x0, y0, min(end * block, width) - x0, min(y0 + block, height) - y0))
            bx = end
    return tiles


def np_classify(film, moment, block_samples, threshold, floor=0.0, max_samples=0, block=0, outlier_permille=0, border=0):
    """The header's pixel and block tests in numpy fp32, one rounding per operation (numpy neither contracts nor flushes): the records, 1-D of BLOCK_DTYPE."""
    f32 = np.float32
    film, moment = np.asarray(film, f32), np.asarray(moment, f32)
    h, w, e = film.shape[0] - 2 * border, film.shape[1] - 2 * border, block or 16
    T, M = film[border:border + h, border:border + w], moment[border:border + h, border:border + w]
    nbx, nby = (w + e - 1) // e, (h + e - 1) // e
    ns = np.asarray(block_samples, np.uint32).reshape(nby, nbx)
    n = np.repeat(np.repeat(ns, e, 0), e, 1)[:h, :w].astype(f32)
    thr2, fl = f32(threshold) * f32(threshold), f32(floor) if floor else f32(0.01)
    with np.errstate(all="ignore"):
        valid = T[..., 3] != 0
        c = T[..., :3] / T[..., 3:4]
        s = np.where(M[..., 3:4] != 0, M[..., :3] / M[..., 3:4], f32(0))
        d = s - c * c
        var = np.where(d > 0, d, f32(0))
        v = ((var[..., 0] + var[..., 1]) + var[..., 2]) / n
        m = (c[..., 0] + c[..., 1]) + c[..., 2]
        a = np.where(m > 0, m, f32(0)) + fl
        noisy = valid & (v > thr2 * (a * a))
    out = np.zeros(nby * nbx, BLOCK_DTYPE)
    for by in range(nby):
        for bx in range(nbx):
            k, nb = by * nbx + bx, int(ns[by, bx])
            if nb == 0:
                continue
            sl = (slice(by * e, min(by * e + e, h)), slice(bx * e, min(bx * e + e, w)))
            nv, nn = int(valid[sl].sum()), int(noisy[sl].sum())
            conv = nn * 1000 <= outlier_permille * nv
            out[k] = (nb, nn, nv, CONVERGED if conv else (AT_CAP if max_samples and nb >= max_samples else 0))
    return out


# ---------------------------------------------------------------- crafted films for the classification stage
def crafted_films(width, height, border, block, threshold, floor=0.0, seed=0):
    """(film, moment, block_samples) that hold the corners of the pixel and block tests, for a frame cut into `block`-pixel blocks. Every pixel starts quiet and valid -
    T = (0, g, 0, 1), M = (0, g g, 0, 1): v = 0 -; every tested block then receives, at random places, one pixel of each corner: w = 0; M.w = 0 with T.w != 0; a negative
    w (Mitchell's lobes); s < c c; v equal to the bound to the last bit and one ulp above it (subnormal both when the threshold is tiny); Inf and NaN channels. The
    blocks' n cycle through 4, 3, 65536, 0 (skipped), 16, 7, and loud pixels (v far above the bound) are added until a block's noisy count - counted with np_classify -
    is exactly half of its valid count, one more than half, zero, or a random number: the bound of outlierPermille = 500 is straddled."""
    f32 = np.float32
    rng = np.random.default_rng(seed)
    e, fl = block, f32(floor) if floor else f32(0.01)
    nbx, nby = (width + e - 1) // e, (height + e - 1) // e
    H, W = height + 2 * border, width + 2 * border
    g = rng.uniform(0.05, 2.0, (H, W)).astype(f32)
    film, moment = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32)
    film[..., 1], film[..., 3] = g, 1
    moment[..., 1], moment[..., 3] = g * g, 1
    ns = np.array([(4, 3, 65536, 0, 16, 7)[(k + seed) % 6] for k in range(nbx * nby)], np.uint32)
    thr2 = f32(threshold) * f32(threshold)
    found = 0
    for k in range(nbx * nby):
        by, bx = divmod(k, nbx)
        px = [(y, x) for y in range(by * e, min(by * e + e, height)) for x in range(bx * e, min(bx * e + e, width))]
        order = [px[i] for i in rng.permutation(len(px))]
        n = f32(max(int(ns[k]), 1))

        def put(T, M):
            y, x = order.pop()
            film[y + border, x + border], moment[y + border, x + border] = T, M

        if len(order) >= 24:
            put((1, 1, 1, 0), (1, 1, 1, 0))                                   # w == 0: not valid
            put((0.5, 0.5, 0.5, 1), (9, 9, 9, 0))                             # M.w == 0: s = 0, quiet
            put((-0.3, -0.2, -0.1, -0.5), (-2, -2, -2, -0.5))                 # negative weights: c and s positive again
            put((-0.3, 0.2, 0.1, -0.5), (5, 5, 5, 0.5))                       # a negative brightness: a = floor
            put((0.9, 0.9, 0.9, 1), (0.5, 0.5, 0.5, 1))                       # s < c c: variance clamped to 0
            put((np.inf, 0.5, 0.5, 1), (1, 1, 1, 1))
            put((0.5, np.nan, 0.5, 1), (1, 1, 1, 1))
            put((0.5, 0.5, 0.5, 1), (np.inf, 1, 1, 1))
            put((0.5, 0.5, 0.5, 1), (1, np.nan, 1, 1))
            put((0.5, 0.5, 0.5, np.nan), (1, 1, 1, 1))
            for above in (False, True):                                       # v == bound, v == the float after the bound
                gg = f32(rng.uniform(0.05, 2.0))
                a = gg + fl
                bound = thr2 * (a * a)
                want = np.nextafter(bound, f32(np.inf)) if above else bound
                x0 = f32(want * n)
                for x in [x0] + [np.nextafter(x0, f32(s * np.inf)) for s in (1, -1)]:
                    if f32(((x + f32(0)) + f32(0)) / n) == want and want > 0:
                        put((0, gg, 0, 1), (x, gg * gg, 0, 1))
                        found += 1
                        break
        # loud pixels until the block's noisy count is the target
        def counts():
            r = np_classify(film, moment, np.where(np.arange(ns.size) == k, max(int(ns[k]), 1), 0), threshold, floor, 0, e, 0, border)[k]
            return int(r["noisy"]), int(r["valid"])
        noisy, valid = counts()
        target = (valid // 2, valid // 2 + 1, 0, int(rng.integers(0, max(valid, 1))))[(k + seed) % 4]
        while noisy < target and order:
            put((0, 1, 0, 1), (1e30, 1, 0, 1))
            noisy += 1
    assert found > 0, "no pixel sits on the bound"
    return film, moment, ns

"""Cases and instruments of the sample-by-sample tests at the corners of the samplers' domain (tests/test_sample_corners_cpu.py, tests/test_sample_corners_gpu.py).

The instrument: under rfilter = {"type": "box", "radius": 0.5} the film has no apron (border == 0), a sample of pixel (x, y) lands in texel (x, y) alone with
weight 1, and a render of the one-sample range [k, k + 1) therefore leaves (r, g, b, 1) of sample k of pixel (x, y) in texel (x, y) - for BOTH pipelines of
kz_render, with no entry point of its own. A render of [b, e) leaves the float32 sum of those values in sample order. test_sample_corners_cpu.py holds the
oracle to exactly that, so that a film that differs on the device is a sample that differs.

The cases reach what the bit-level tests of test_gpu_parity.py (1 .. 16 samples per pixel, seeds below 100) never do: sample counts and indices up to the
declared limit of 65536, counts that are a power of 4, a power of 2 only, and neither (permuteIdx with and without its modulo, next1D with and without invSpp),
seeds with bits above 31 (the tail bytes of Hash(p, dim, seed)), waves of one pixel (S a multiple of 64: the first-lane pixel of kz_wf_generate), the
dimension counter of deep paths (wfPmjDim, the first-lane counter of wfLoadSampler), and pixels past the blue-noise period and the pmj pixel tile."""
import collections

import numpy as np

BOX = {"type": "box", "radius": 0.5}
W, H = 40, 24                                     # 960 paths per sample: 15 waves, the last rows of a 256-lane block ragged
SAMPLERS = ("independent", "stratified", "correlated", "pmj02bn")
SEEDS = (7, 2 ** 31 + 5, 2 ** 32 - 1, 0x9E3779B97F4A7C15)
HIGH_WORD = 0x5bd1e995 << 32                      # what the seed-sensitivity check flips: bits 32 .. 63 only
REQUESTED = (1, 100, 1000, 2048, 4097, 65536)
# the counts after each constructor's rounding (Stratified: the next square from resolution 4 on, sampler.cpp:84-92; Correlated: ceil(n / floor(sqrt n)) * floor(sqrt n),
# sampler.cpp:179-187; pmj02bn: capped at 65536): 65536 = 4^8 and 1024 = 4^5, 2048 = 2^11 only (independent and pmj02bn: a square or r0 * r1 with r0 - r1 <= 2 is
# never such a count), the others neither
ROUNDED = {"independent": (1, 100, 1000, 2048, 4097, 65536), "pmj02bn": (1, 100, 1000, 2048, 4097, 65536),
           "stratified": (16, 100, 1024, 2116, 4225, 65536), "correlated": (1, 100, 1023, 2070, 4160, 65536)}

Case = collections.namedtuple("Case", "id sampler requested count seed setting")


# counts beside REQUESTED that a table asks for, with what every constructor makes of them: 4096 = 64^2 = 64 * 64 = 4^6 is left alone by all four
EXTRA_COUNTS = {4096: {s: 4096 for s in SAMPLERS}}


def _case(sampler, requested, seed, setting="cornell"):
    if requested not in REQUESTED and requested not in EXTRA_COUNTS:
        raise ValueError("sample count %d: neither in REQUESTED nor in EXTRA_COUNTS, so its rounded count is not stated" % requested)
    count = ROUNDED[sampler][REQUESTED.index(requested)] if requested in REQUESTED else EXTRA_COUNTS[requested][sampler]
    return Case("%s-%d-seed%x%s" % (sampler, requested, seed, "" if setting == "cornell" else "-" + setting), sampler, requested, count, seed, setting)


# every sampler x every count; the seed moves one step per sampler and per count, so every sampler meets all four seeds
COUNT_CASES = [_case(s, n, SEEDS[(i + j) % 4]) for i, s in enumerate(SAMPLERS) for j, n in enumerate(REQUESTED)]
# ranges of whole waves of one pixel: [0, 64), [n - 64, n), [n - 128, n)
WAVE_CASES = [_case(s, n, SEEDS[(i + j + 1) % 4]) for i, s in enumerate(SAMPLERS) for j, n in enumerate((4096, 65536))]
# the dimension counter: maxDepth 12 at count 100 - pmj02bn instances >= 5 (the permuted index), the roulette dimension of bounces > 3
# (sphere_env's paths end at their second vertex - the sphere is convex and alone - so box_env states the nLights == 0 term for deep paths: the cornell box, whose front
# is open, with its light switched off under a white background)
SETTINGS = ("reg_on", "reg_off", "thinlens", "sphere_env", "light_invisible", "light_visible", "box_env")
DIM_CASES = [_case(s, 100, SEEDS[(i + j) % 4], st) for i, s in enumerate(SAMPLERS) for j, st in enumerate(SETTINGS)]
DIM_KS = (0, 63, 99)
DIM_RANGE = (36, 100)
# pixel coordinates past the 128-texel blue-noise period, past the pmj pixel tile, the last row and column
BIG_W, BIG_H, BIG_K = 2048, 1536, 999
BIG_TILES = [(2040, 1528, 8, 8), (120, 120, 16, 16), (0, 1530, 5, 6)]
BIG_CASES = [_case("pmj02bn", 1000, SEEDS[2], "big"), _case("independent", 1000, SEEDS[3], "big")]
# pass schedules and camera-ray kernels at the last index of the largest count
SCHEDULE_CASES = [_case(s, 65536, SEEDS[(i + 2) % 4]) for i, s in enumerate(SAMPLERS)]
SCHEDULES = ({"pass_items": 64}, {"pass_items": 4096, "passes_in_flight": 3}, {"tune": {"packetPrimary": 0}}, {"tune": {"packetPrimary": 1}}, {"tune": {"packetPrimary": 2}})


def sample_indices(n):
    """k in {0, 1, 63, 64, n/2, n-2, n-1}, clipped to the count."""
    return sorted({k for k in (0, 1, 63, 64, n // 2, n - 2, n - 1) if 0 <= k < n})


def wave_ranges(n):
    return [(0, 64), (n - 64, n), (n - 128, n)]


def box_scene(desc):
    """The description under the box filter of radius 0.5: border == 0, one texel per sample, weight 1."""
    desc.camera["rfilter"] = dict(BOX)
    return desc


def scene_of(S, case):
    """The case's description (S: the package's scenes module)."""
    sampler = {"type": case.sampler, "sampleCount": case.requested, "seed": case.seed}
    if case.setting == "big":
        d = S.cornell_box(BIG_W, BIG_H, case.requested, sampler=case.sampler, seed=case.seed)
    elif case.setting == "sphere_env":
        d = S.sphere_env(W, H, case.requested)                         # no lights, a background: the nLights == 0 term of wfPmjDim
    else:
        d = S.cornell_box(W, H, case.requested, sampler=case.sampler, seed=case.seed)
    d.sampler = sampler
    if case.setting != "cornell" and case.setting != "big":
        d.integrator.update(maxDepth=12, regularization=(case.setting == "reg_on"))
    if case.setting == "thinlens":
        d.camera.update(type="thinlens", apertureRadius=0.1, focusDistance=3.5)
    if case.setting == "box_env":
        d.meshes = [dict(m, light=None) for m in d.meshes]
        d.background = {"color": (1.0, 1.0, 1.0), "intensity": 1.0}
    if case.setting in ("light_invisible", "light_visible"):           # invisible: the walk-through continuation of a camera ray that meets the light first
        for m in d.meshes:
            if m["light"]:
                m["light"] = dict(m["light"], lightPrimaryVisibility=(case.setting == "light_visible"))
    return box_scene(d)


def with_seed(desc, seed):
    desc.sampler = dict(desc.sampler, seed=seed)
    return desc


def _is_oracle(obj):
    return hasattr(obj, "render_canonical")


def range_film(obj, begin, end, tiles=None, **render_kw):
    """The film of the sample range [begin, end) from a Scene (kz_render with render_kw: pipeline, pass_items, tune, ...) or from an OracleScene (render_canonical)."""
    if _is_oracle(obj):
        return obj.render_canonical(begin, end, tiles=tiles, threads=0)
    obj.render(begin, end, tiles=tiles, **render_kw)
    return obj.film()


def one_sample_films(obj, ks, tiles=None, **render_kw):
    """{k: the film of the one-sample range [k, k + 1)}: under the box filter, texel (x, y) = (r, g, b, 1) of sample k of pixel (x, y)."""
    return {k: range_film(obj, k, k + 1, tiles=tiles, **render_kw) for k in ks}


def pixel_grid(w=W, h=H, tiles=None):
    """(n, 2) int32: every pixel of the frame (or of the tiles), row-major."""
    if tiles is None:
        tiles = [(0, 0, w, h)]
    out = []
    for x0, y0, tw, th in tiles:
        yy, xx = np.meshgrid(np.arange(y0, y0 + th), np.arange(x0, x0 + tw), indexing="ij")
        out.append(np.stack([xx.ravel(), yy.ravel()], 1))
    return np.concatenate(out).astype(np.int32)


def samples_of(obj, pxy, k):
    """render_samples of sample k of every pixel of pxy: (n, 5) = position x, y, radiance r, g, b."""
    return obj.render_samples(pxy, np.full(len(pxy), k, np.uint32))


def valid(rows):
    """Color3f::isValid on render_samples rows: no component negative, infinite or NaN (ImageBlock::put drops the others with their weight)."""
    c = rows[:, 2:5]
    return (np.isfinite(c) & ~(c < 0)).all(axis=1)


def on_edge(rows, pxy):
    """Samples whose position is not strictly inside their pixel: a jitter component of exactly 0 (the box of radius 0.5 then reaches two texels) or one that
    rounds up to the next pixel when added to the pixel's coordinate. The film comparison covers them; the one-texel identity does not."""
    j = rows[:, :2] - pxy.astype(np.float32)
    return ((j <= 0) | (j >= 1)).any(axis=1)


def edge_texels(rows_per_sample, pxy, w=W, h=H):
    """(h, w) bool: the texels an on-edge sample of these rows can reach - its own pixel and the eight around it. Everything else is one texel per sample."""
    mask = np.zeros((h, w), bool)
    for rows in rows_per_sample:
        e = on_edge(rows, pxy)
        for x, y in pxy[e]:
            mask[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    return mask


def film_of_samples(rows_per_sample, pxy, w=W, h=H):
    """The box film the rows imply: per pixel, 0 + (r, g, b, 1) of every valid sample, added in sample order in float32 (what ImageBlock::put and the fixed order of
    the tap sums come to when every weight is 1). rows_per_sample: one render_samples array per sample of the range, in order."""
    film = np.zeros((h, w, 4), np.float32)
    x, y = pxy[:, 0], pxy[:, 1]
    for rows in rows_per_sample:
        ok = valid(rows)
        add = np.concatenate([rows[:, 2:5], np.ones((len(rows), 1), np.float32)], 1).astype(np.float32)
        add[~ok] = 0
        film[y, x] = film[y, x] + add                                   # (pxy holds every pixel once: a plain gather / scatter)
    return film


def differing_words(a, b):
    """Indices (rows of the first axis pair) where two float32 arrays differ in a bit: two NaNs count as equal, +0 and -0 do not."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


def _hex(v):
    v = np.ascontiguousarray(v, np.float32)
    return "(" + ", ".join("%.9g [%08x]" % (float(x), int(b)) for x, b in zip(v.ravel(), v.view(np.uint32).ravel())) + ")"


def _head(case, ora, what):
    return "%s: sampler %s, count %d (asked %d), seed 0x%x, %s" % (what, case.sampler, ora.sample_count, case.requested, case.seed, case.setting)


def report(case, ora, begin, end, got, want, what, limit=4):
    """What a failing film comparison says: for (the first `limit` of) the texels that differ, the pixel, the sample index or range, sampler, count and seed, the
    device's texel, the oracle's, and the oracle's render_samples row of the range's first sample with its jitter."""
    bad = differing_words(got, want).any(axis=2)
    ys, xs = np.nonzero(bad)
    lines = [_head(case, ora, what) + ": %d of %d texels differ over samples [%d, %d)" % (len(xs), bad.size, begin, end)]
    for x, y in list(zip(xs, ys))[:limit]:
        row = ora.render_samples(np.array([[x, y]], np.int32), np.array([begin], np.uint32))[0]
        lines.append("  pixel (%d, %d) sample %s: device %s oracle film %s | oracle render_samples(%d) position (%.9g, %.9g) jitter (%.9g, %.9g) radiance %s"
                     % (x, y, begin if end == begin + 1 else "%d..%d" % (begin, end - 1), _hex(got[y, x]), _hex(want[y, x]), begin, row[0], row[1],
                        row[0] - np.float32(x), row[1] - np.float32(y), _hex(row[2:5])))
    return "\n".join(lines)


def report_samples(case, ora, pxy, k, got, want, what, limit=4):
    """The same for a render_samples comparison: the rows that differ, with pixel, sample index, sampler, count and seed."""
    bad = np.nonzero(differing_words(got, want).any(axis=1))[0]
    lines = [_head(case, ora, what) + ": %d of %d samples differ at index %d" % (len(bad), len(pxy), k)]
    for i in bad[:limit]:
        x, y = int(pxy[i, 0]), int(pxy[i, 1])
        lines.append("  pixel (%d, %d) sample %d: device position %s radiance %s | oracle position %s radiance %s jitter (%.9g, %.9g)"
                     % (x, y, k, _hex(got[i, :2]), _hex(got[i, 2:5]), _hex(want[i, :2]), _hex(want[i, 2:5]), want[i, 0] - np.float32(x), want[i, 1] - np.float32(y)))
    return "\n".join(lines)

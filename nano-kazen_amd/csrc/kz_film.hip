// kz_film.hip - the film: deterministic ImageBlock::put (block.cpp:56-96) as HIP kernels for gfx950, the packing / download of tile rects
// (the device half of the multi-GPU gather), the 8-bit sRGB resolve, and the kz_film_* entry points.
#include "kz_state.h"
#include "../../include/kazen_mi355x_variance.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "kz_devfn.h"

// ============================================================================================
// a25 ImageBlock::put (block.cpp:56-96) as RUNNING TAP SUMS (round 6). For every pixel of the frame the replica keeps taps x taps accumulators
// (rgb * w, w) - one per film texel the pixel's samples can reach - laid out tap-major over the frame, [tap][y * width + x]:
//   kz_film_taps      after every pass: one wave per 64 / GROUPS consecutive pixels of the pass's pixel list. It LOADS the pixel's accumulators, adds the
//                     pass's samples of that pixel in sample order - validity (Color3f::isValid), the separable filter weights of block.cpp:64-80 per tap,
//                     the weighted products of block.cpp:84 - and stores them back. An accumulator is therefore the sum, in sample order, of everything
//                     the pixel has been given since the film was cleared, WHATEVER passes, calls, contexts or batches brought the samples: the grouping of
//                     the float additions no longer depends on the pass size, on how fast the pass context grew, on the number of passes in flight (H10).
//   kz_film_resolve   once per call: film texel = sum, over the cells of the canonical tile grid (G x G pixels, row-major) its footprint touches, of the
//                     cell's partial sum (taps in (row, column) order). This is exactly what the host merge of per-tile rects forms (ImageBlock::put(ImageBlock&)
//                     in tile order), so the film of one device, of N devices with tiles dealt beforehand and of N devices taking batches from a counter are
//                     the same bits when the tiles are the grid's.
//   kz_film_tile_rects the packed rect of a tile (the tile with its filter apron, the extent of an ImageBlock): the partial sums of THAT tile's pixels only.
// The weights are formed block-relative exactly as the reference does (32x32 blocks at multiples of KAZEN_BLOCK_SIZE), so they are bit-identical to
// ImageBlock::put; only the order of the float additions is the build's own (fixed) one.
// ============================================================================================
// GROUPS lane groups share a pixel: group g carries the tap ROWS [g * R0, g * R0 + R0) of its 64 / GROUPS pixels, R0 = ceil(TAPS / GROUPS). Every accumulator
// receives the same products in the same (sample) order whatever GROUPS is; what is paid for more groups is the per-sample set-up (validity, footprint, the
// x weights) once per group. TAPS <= 5 (every default of the reference): two groups - 15 and 10 accumulators instead of 25, 10.5 KB of staging per wave
// (round 5: film stage of a 2^30-item pass of C4 12.6 -> 10.5 ms); 6 .. 9 taps (radius up to 4): four groups, at most 27 accumulators per lane.
// SIGNED (compile time): the values are a feature film's (kazen_mi355x_aov.h) - a normal has negative components - so the sign half of Color3f::isValid is
// skipped and the isfinite half kept. The picture's instantiations (SIGNED = false) keep the code they had.
template <int TAPS, int GROUPS, bool SIGNED = false>
__global__ __launch_bounds__(64) void kz_film_taps(KzParams P, const float *__restrict__ filter, const uint32_t *__restrict__ pixList, uint32_t nPix, uint32_t S,
                                                   const float *__restrict__ inJx, const float *__restrict__ inJy, const float *__restrict__ inR,
                                                   const float *__restrict__ inG, const float *__restrict__ inB, float4 *__restrict__ tapSums, size_t framePix) {
    constexpr int PIX = 64 / GROUPS, R0 = (TAPS + GROUPS - 1) / GROUPS, CHUNK = GROUPS == 1 ? KZ_TAPS_CHUNK1 : KZ_TAPS_CHUNK;
    __shared__ float s_filter[KZ_FILTER_RESOLUTION + 1];
    __shared__ float s_in[5][CHUNK][PIX + 1];                          // [array][sample][pixel], rows padded against bank conflicts of the transposing store
    const int lane = threadIdx.x, pixLane = lane % PIX, group = lane / PIX;
    if (lane <= KZ_FILTER_RESOLUTION) s_filter[lane] = filter[lane];
    const uint32_t pl0 = blockIdx.x * (uint32_t)PIX, pl = pl0 + (uint32_t)pixLane;
    const bool havePixel = pl < nPix;
    const uint32_t pxy = havePixel ? pixList[pl] : 0u;
    const int px = (int)(pxy & 0xffffu), py = (int)(pxy >> 16);
    const int bx0 = px & ~31, by0 = py & ~31;                          // the reference block this pixel is rendered in
    const float r = P.filterRadius, lf = P.lookupFactor;
    const int ty0 = group * R0, nRowsMine = min(R0, max(0, TAPS - ty0));
    float xb[TAPS], yb[R0];                                            // block-relative film coordinates this pixel reaches through tap t
#pragma unroll
    for (int t = 0; t < TAPS; ++t) xb[t] = (float)(px + P.border - P.tapLo - t - bx0);
#pragma unroll
    for (int t = 0; t < R0; ++t) yb[t] = (float)(py + P.border - P.tapLo - (ty0 + t) - by0);
    float4 *const mine = tapSums + (size_t)py * (size_t)P.width + (size_t)px;
    float4 acc[R0 * TAPS];
#pragma unroll
    for (int ty = 0; ty < R0; ++ty)
#pragma unroll
        for (int tx = 0; tx < TAPS; ++tx)
            acc[ty * TAPS + tx] = (havePixel && ty < nRowsMine) ? mine[(size_t)((ty0 + ty) * TAPS + tx) * framePix] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float *const in[5] = {inJx, inJy, inR, inG, inB};
    const uint32_t nRows = min((uint32_t)PIX, nPix - min(nPix, pl0));  // pixels of this wave
    for (uint32_t c0 = 0; c0 < S; c0 += CHUNK) {
        const uint32_t n = min((uint32_t)CHUNK, S - c0);
        __syncthreads();
        for (uint32_t i = lane; i < nRows * CHUNK; i += 64u) {         // consecutive lanes: consecutive samples of one pixel, then the next pixel
            const uint32_t p = i / CHUNK, k = i % CHUNK;
            if (k < n) {
                const size_t gi = (size_t)(pl0 + p) * S + c0 + k;
#pragma unroll
                for (int a = 0; a < 5; ++a) s_in[a][k][p] = in[a][gi];
            }
        }
        __syncthreads();
        if (havePixel) {
            for (uint32_t k = 0; k < n; ++k) {
                const float jx = s_in[0][k][pixLane], jy = s_in[1][k][pixLane];
                const float cr = s_in[2][k][pixLane], cg = s_in[3][k][pixLane], cb = s_in[4][k][pixLane];
                const bool valid = (SIGNED || (cr >= 0.f && cg >= 0.f && cb >= 0.f)) && isfinite(cr) && isfinite(cg) && isfinite(cb);   // Color3f::isValid
                if (!valid) continue;                                  // an invalid sample carries weight 0 everywhere: adds exact zeros
                const float posx = ((float)px + jx) - 0.5f - (float)(bx0 - P.border), posy = ((float)py + jy) - 0.5f - (float)(by0 - P.border);   // block.cpp:64-67
                const float lox = ceilf(posx - r), hix = floorf(posx + r), loy = ceilf(posy - r), hiy = floorf(posy + r);                     // block.cpp:70-73
                float wx[TAPS], wy[R0];
#pragma unroll
                for (int t = 0; t < TAPS; ++t) wx[t] = !(xb[t] < lox || xb[t] > hix) ? s_filter[(int)(fabsf(xb[t] - posx) * lf)] : 0.f;          // block.cpp:77-80
#pragma unroll
                for (int t = 0; t < R0; ++t) wy[t] = (t < nRowsMine && !(yb[t] < loy || yb[t] > hiy)) ? s_filter[(int)(fabsf(yb[t] - posy) * lf)] : 0.f;
#pragma unroll
                for (int ty = 0; ty < R0; ++ty)
#pragma unroll
                    for (int tx = 0; tx < TAPS; ++tx) {
                        float4 &a = acc[ty * TAPS + tx];
                        a.x += cr * wx[tx] * wy[ty]; a.y += cg * wx[tx] * wy[ty]; a.z += cb * wx[tx] * wy[ty]; a.w += 1.0f * wx[tx] * wy[ty];     // block.cpp:84
                    }
            }
        }
    }
    if (havePixel) {
#pragma unroll
        for (int ty = 0; ty < R0; ++ty)
            if (ty < nRowsMine) {
#pragma unroll
                for (int tx = 0; tx < TAPS; ++tx) mine[(size_t)((ty0 + ty) * TAPS + tx) * framePix] = acc[ty * TAPS + tx];
            }
    }
}

// The partial sum a film texel receives from the source pixels [xa, xb] x [ya, yb] (all inside the texel's footprint, whose first source column / row is
// x0s / y0s): taps in (row, column) order. Shared by the two kernels below - they must form the same bits.
__device__ __forceinline__ float4 kzTapPartial(const float4 *__restrict__ tapSums, size_t framePix, int width, int taps, int x0s, int y0s, int xa, int xb, int ya, int yb) {
    float4 part = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int y = ya; y <= yb; ++y)
        for (int x = xa; x <= xb; ++x) {
            const float4 t = tapSums[(size_t)((y - y0s) * taps + (x - x0s)) * framePix + (size_t)y * (size_t)width + (size_t)x];
            part.x += t.x; part.y += t.y; part.z += t.z; part.w += t.w;
        }
    return part;
}

// film texel = sum over the grid cells its footprint touches (row-major) of that cell's partial: ImageBlock::put(ImageBlock&) (block.cpp:87-96) of the
// cells' blocks in tile order. Every texel of the film is written (zero where nothing reaches it).
__global__ __launch_bounds__(256) void kz_film_resolve(KzParams P, const float4 *__restrict__ tapSums, size_t framePix, int G, float4 *__restrict__ film) {
    const int cols = P.width + 2 * P.border, rows = P.height + 2 * P.border;
    const int fx = blockIdx.x * 16 + (threadIdx.x & 15), fy = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (fx >= cols || fy >= rows) return;
    const int taps = P.tapHi - P.tapLo + 1;
    const int x0s = fx - P.border + P.tapLo, y0s = fy - P.border + P.tapLo;      // the source pixel that reaches this texel through tap (0, 0)
    const int xlo = max(x0s, 0), xhi = min(x0s + taps - 1, P.width - 1), ylo = max(y0s, 0), yhi = min(y0s + taps - 1, P.height - 1);
    float4 total = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xlo <= xhi && ylo <= yhi) {
        for (int tr = ylo / G; tr <= yhi / G; ++tr)
            for (int tc = xlo / G; tc <= xhi / G; ++tc) {
                const float4 part = kzTapPartial(tapSums, framePix, P.width, taps, x0s, y0s, max(xlo, tc * G), min(xhi, tc * G + G - 1), max(ylo, tr * G), min(yhi, tr * G + G - 1));
                total.x += part.x; total.y += part.y; total.z += part.z; total.w += part.w;
            }
    }
    film[(size_t)fy * cols + fx] = total;
}

// The film rects of a tile list, packed: tile t contributes its (h + 2b) x (w + 2b) rect (the tile with its filter apron) as consecutive rows at
// rects[t].offset (in float4s), each texel = what the TILE'S OWN pixels add to it - an ImageBlock of the tile. The aprons of neighbouring tiles overlap in
// the film; the merge adds them there. One workgroup per (tile, row).
__global__ __launch_bounds__(128) void kz_film_tile_rects(KzParams P, const float4 *__restrict__ tapSums, size_t framePix, const KzTileRect *__restrict__ rects,
                                                          float4 *__restrict__ out, uint32_t nTiles) {
    const uint32_t tile = blockIdx.y + blockIdx.z * 65535u;             // (a grid's y extent ends at 65535: longer tile lists continue in z)
    if (tile >= nTiles) return;
    const KzTileRect r = rects[tile];
    const int rw = r.w + 2 * P.border, rh = r.h + 2 * P.border;
    const int row = blockIdx.x;
    if (row >= rh) return;
    const int taps = P.tapHi - P.tapLo + 1;
    const int fy = r.y0 + row, y0s = fy - P.border + P.tapLo;
    const int ya = max(y0s, r.y0), yb = min(y0s + taps - 1, r.y0 + r.h - 1);
    float4 *dst = out + r.offset + (size_t)row * rw;
    for (int x = threadIdx.x; x < rw; x += blockDim.x) {
        const int x0s = r.x0 + x - P.border + P.tapLo;
        dst[x] = kzTapPartial(tapSums, framePix, P.width, taps, x0s, y0s, max(x0s, r.x0), min(x0s + taps - 1, r.x0 + r.w - 1), ya, yb);
    }
}


// Film -> 8-bit sRGB raster: Color4f::divideByFilterWeight (color.h:94-99), Color3f::toSRGB (common.cpp:351-366) and the
// clamp + truncation of Bitmap::savePNG (bitmap.cpp:45-52). One pixel per lane, coalesced float4 reads.
__global__ void kz_film_srgb8(const float4 *__restrict__ film, int width, int height, int border, uint8_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)(width * height)) return;
    const int y = (int)(i / (uint32_t)width), x = (int)(i - (uint32_t)y * (uint32_t)width);
    const float4 px = film[(size_t)(y + border) * (size_t)(width + 2 * border) + (size_t)(x + border)];
    float c[3] = {0.f, 0.f, 0.f};
    if (px.w != 0.f) { c[0] = px.x / px.w; c[1] = px.y / px.w; c[2] = px.z / px.w; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = c[k];
        const float t = v <= 0.0031308f ? 12.92f * v : (1.0f + 0.055f) * kzPow(v, 1.0f / 2.4f) - 0.055f;
        const float s = 255.f * t;
        out[3 * (size_t)i + k] = (uint8_t)(s < 0.f ? 0.f : (s > 255.f ? 255.f : s));
    }
}

// Before the passes of a call (renderOn), and before a film's rects are packed (downloadTiles): KzFilm::ensure with the scene's geometry - taps^2 float4 of sums per
// pixel of the frame (C4, 5 taps: 829 MB; C5: 3.3 GB), allocated and zeroed on first use outside the pass contexts' budget.
int kzFilmEnsure(KzScene *scene, KzFilm &film, size_t filmPixels, bool accumulate, hipStream_t stream) {
    const KzParams &P = scene->prm;
    const size_t taps = (size_t)(P.tapHi - P.tapLo + 1), nSums = taps * taps * (size_t)P.width * (size_t)P.height;
    const bool fresh = !film.sums;
    if (fresh) KZ_TRACE("film: tap sums, %.0f MB ...", nSums * sizeof(float4) / 1e6);
    const int rc = film.ensure(nSums, filmPixels, accumulate, stream);
    if (fresh && !rc) KZ_TRACE("film: ... there");
    return rc;
}

int kzFilmClear(KzDeviceState *ds, hipStream_t stream) {
    for (KzFilm &film : ds->films) if (const int rc = film.clear(stream)) return rc;      // the picture, then the feature films, then the second-moment film
    ds->pictureSamples = ds->momentSamples = 0;
    ds->adValid = false;                                                 // (the block records of an adaptive call, kazen_mi355x_adaptive.h: they described the film that went)
    return kzMatteClear(ds, stream);                                     // (the ID-matte tables, kazen_mi355x_matte.h: nothing where there are none)
}

// The film stage of one pass (kz_render.hip: launchWhole / launchHalves for the picture, wfAov once per enabled feature film): ImageBlock::put for every sample record
// of the pass - its five planes jx | jy | r | g | b - into `film`'s running tap sums of the pass's pixels. The kernel reads and writes those sums, so it waits for the
// film stage of the pass before it (`waitFilm`, passes on other streams; null: same stream). isSigned: kz_film_taps<.., SIGNED = true>, a feature film's values.
// lanesPerPixel: 0 = default (2 lane groups per pixel up to 5 taps, 4 beyond), 1 = one lane per pixel (round 2's kernel; up to 5 taps) - the same sums bit for bit.
template <bool SIGNED>
static int launchTaps(const KzParams &P, KzDeviceState *ds, hipStream_t pst, const uint32_t *pixList, uint32_t nPixPass, uint32_t Sp, const float *sJx, const float *sJy,
                      const float *sR, const float *sG, const float *sB, float4 *tapSums, int lanesPerPixel) {
    const int ftaps = P.tapHi - P.tapLo + 1;
    const size_t framePix = (size_t)P.width * (size_t)P.height;
#define KZ_FILM_TAPS(N, GR) hipLaunchKernelGGL((kz_film_taps<N, GR, SIGNED>), dim3((nPixPass + 64 / GR - 1) / (64 / GR)), dim3(64), 0, pst, P, ds->T.filter, pixList, nPixPass, Sp, sJx, sJy, sR, sG, sB, tapSums, framePix)
    if (lanesPerPixel == 1 && ftaps <= 5) switch (ftaps) { case 1: KZ_FILM_TAPS(1, 1); break; case 2: KZ_FILM_TAPS(2, 1); break; case 3: KZ_FILM_TAPS(3, 1); break; case 4: KZ_FILM_TAPS(4, 1); break; default: KZ_FILM_TAPS(5, 1); break; }
    else switch (ftaps) {
        case 1: KZ_FILM_TAPS(1, 2); break; case 2: KZ_FILM_TAPS(2, 2); break; case 3: KZ_FILM_TAPS(3, 2); break; case 4: KZ_FILM_TAPS(4, 2); break; case 5: KZ_FILM_TAPS(5, 2); break;
        case 6: KZ_FILM_TAPS(6, 4); break; case 7: KZ_FILM_TAPS(7, 4); break; case 8: KZ_FILM_TAPS(8, 4); break; case 9: KZ_FILM_TAPS(9, 4); break;
        default: return kz_fail(KZ_ERR_UNSUPPORTED, "film filter of %d taps per axis (at most %d)", ftaps, KZ_MAX_FILTER_TAPS);
    }
#undef KZ_FILM_TAPS
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}
int kzFilmStage(KzScene *scene, KzDeviceState *ds, KzFilm &film, bool isSigned, hipStream_t pst, const uint32_t *pixList, uint32_t nPixPass, uint32_t Sp, const float *const plane[5], hipEvent_t waitFilm, int lanesPerPixel) {
    if (waitFilm) HIP_TRY(hipStreamWaitEvent(pst, waitFilm, 0));
    // (the picture's instantiations first: the code the compiler gives the 9-tap kernels follows the order in which the two sets are instantiated)
    return (!isSigned ? launchTaps<false> : launchTaps<true>)(scene->prm, ds, pst, pixList, nPixPass, Sp, plane[0], plane[1], plane[2], plane[3], plane[4], film.sums, lanesPerPixel);
}

// The texels of a film from its tap sums, on `stream` behind whatever fed the sums: ImageBlock::put(ImageBlock&) of the canonical grid's tiles in tile order. The picture's:
// once per call, behind every pass; a feature film's: where it is read (kz_aov_download, kz_denoise). Sums and texels are there.
int kzFilmResolve(KzScene *scene, KzFilm &film, hipStream_t stream) {
    const KzParams &P = scene->prm;
    const int cols = P.width + 2 * P.border, rows = P.height + 2 * P.border;
    hipLaunchKernelGGL(kz_film_resolve, dim3((cols + 15) / 16, (rows + 15) / 16), dim3(256), 0, stream, P, (const float4 *)film.sums, (size_t)P.width * (size_t)P.height, KZ_FILM_GRID, film.texels);
    HIP_TRY(hipGetLastError());
    return KZ_OK;
}

// Floats of the packed film rects of a tile list: tile t holds (h + 2b) x (w + 2b) x 4 floats - the tile with its filter apron.
size_t packedFloats(const KzParams &P, const KzTile *tiles, uint32_t nTiles) {
    size_t n = 0;
    for (uint32_t t = 0; t < nTiles; ++t) n += (size_t)(tiles[t].w + 2 * P.border) * (size_t)(tiles[t].h + 2 * P.border) * 4;
    return n;
}
int checkTiles(const KzParams &P, const KzTile *tiles, uint32_t nTiles) {
    if (!tiles && nTiles) return kz_fail(KZ_ERR_INVALID_ARG, "null tile list");
    for (uint32_t t = 0; t < nTiles; ++t) {
        const KzTile &tl = tiles[t];
        if (tl.x0 < 0 || tl.y0 < 0 || tl.w <= 0 || tl.h <= 0 || tl.x0 + tl.w > P.width || tl.y0 + tl.h > P.height)
            return kz_fail(KZ_ERR_INVALID_ARG, "tile %u (%d,%d %dx%d) outside the %dx%d image", t, tl.x0, tl.y0, tl.w, tl.h, P.width, P.height);
    }
    return KZ_OK;
}

// the rects of `tiles` of film `film` of replica ds -> host `packed` (through a device-side pack and a pinned staging buffer: one D2H copy at link rate)
int downloadTiles(KzScene *scene, KzDeviceState *ds, KzFilm &film, const KzTile *tiles, uint32_t nTiles, float *packed, size_t nFloats, hipStream_t stream) {
    const KzParams &P = scene->prm;
    int rc;
    if ((rc = checkTiles(P, tiles, nTiles))) return rc;
    const size_t need = packedFloats(P, tiles, nTiles);
    if (!packed || nFloats != need) return kz_fail(KZ_ERR_INVALID_ARG, "packed tile buffer must hold %zu floats (kz_tiles_packed_floats)", need);
    if (nTiles == 0) return KZ_OK;
    std::vector<KzTileRect> rects(nTiles);
    size_t off = 0; int maxRows = 0;
    for (uint32_t t = 0; t < nTiles; ++t) {
        rects[t] = KzTileRect{tiles[t].x0, tiles[t].y0, tiles[t].w, tiles[t].h, (uint32_t)off};
        off += (size_t)(tiles[t].w + 2 * P.border) * (size_t)(tiles[t].h + 2 * P.border);
        maxRows = std::max(maxRows, tiles[t].h + 2 * P.border);
    }
    if (off >= (1ull << 32)) return kz_fail(KZ_ERR_UNSUPPORTED, "tile set of %zu film pixels (limit 2^32)", off);
    if (nTiles > ds->rectsDev.cap() && (rc = ds->rectsDev.regrow(nTiles))) return rc;
    if (off > ds->packDev.cap() && (rc = ds->packDev.regrow(off + off / 8))) return rc;      // (headroom: the next tile set of about this size reuses the buffers)
    if (off > ds->packHost.cap()) (void)ds->packHost.regrow(off + off / 8);                  // (no pinned memory to be had: the copy below goes to the caller's pageable buffer)
    HIP_TRY(hipMemcpyAsync(ds->rectsDev, rects.data(), (size_t)nTiles * sizeof(KzTileRect), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));                              // (the tables are host vectors of this call)
    if (nTiles > 65535u * 65535u) return kz_fail(KZ_ERR_UNSUPPORTED, "kz_film_download_tiles: %u tiles in one call", nTiles);
    const unsigned gz = (nTiles + 65534u) / 65535u, gy = gz > 1 ? 65535u : nTiles;
    if ((rc = kzFilmEnsure(scene, film, ds->filmPixels, true, stream))) return rc;      // (a replica nothing has been rendered on: zeros)
    hipLaunchKernelGGL(kz_film_tile_rects, dim3((unsigned)maxRows, gy, gz), dim3(128), 0, stream, P, (const float4 *)film.sums, (size_t)P.width * (size_t)P.height, (const KzTileRect *)ds->rectsDev.get(),
                       ds->packDev.get(), nTiles);
    HIP_TRY(hipGetLastError());
    if (ds->packHost) {
        HIP_TRY(hipMemcpyAsync(ds->packHost, ds->packDev, off * sizeof(float4), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        std::memcpy(packed, ds->packHost, off * sizeof(float4));
    } else {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(packed, ds->packDev, off * sizeof(float4), hipMemcpyDeviceToHost));
    }
    return KZ_OK;
}

extern "C" {

int kz_tiles_packed_floats(const KzScene *scene, const KzTile *tiles, uint32_t nTiles, size_t *nFloats) {
    if (!scene || !nFloats) return kz_fail(KZ_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = checkTiles(scene->prm, tiles, nTiles))) return rc;
    *nFloats = packedFloats(scene->prm, tiles, nTiles);
    return KZ_OK;
}

int kz_film_download_tiles(KzScene *scene, int device, const KzTile *tiles, uint32_t nTiles, float *packed, size_t nFloats) {
    KzDeviceState *ds; int rc;
    if ((rc = kzAovRefuseGather(scene, "kz_film_download_tiles")) || (rc = kzVarianceRefuseGather(scene, "kz_film_download_tiles")) ||
        (rc = kzMatteRefuseGather(scene, "kz_film_download_tiles")) || (rc = findReplica(scene, device, &ds))) return rc;
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    return downloadTiles(scene, ds, ds->picture(), tiles, nTiles, packed, nFloats, ds->lastStream);
}

int kz_film_clear_on(KzScene *scene, int device, void *stream) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    return kzFilmClear(ds, (hipStream_t)stream);
}
int kz_film_clear(KzScene *scene, void *stream) { return kz_film_clear_on(scene, -1, stream); }

// What the two film downloads share: the buffer's size, the wait for the replica's queued work, the copy of the texels. `resolved`: the texels are current (the picture's:
// every render ends with their resolve); otherwise - a feature film - they are resolved first, and a film nothing has been rendered into yet is zeros.
static int downloadFilm(KzScene *scene, KzDeviceState *ds, KzFilm &film, bool resolved, float *out, size_t nFloats) {
    if (!out || nFloats != ds->filmPixels * 4) return kz_fail(KZ_ERR_INVALID_ARG, "film buffer must hold %zu floats", ds->filmPixels * 4);
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    if (!resolved) {
        if (!film.sums || !film.texels) { std::memset(out, 0, nFloats * sizeof(float)); return KZ_OK; }      // (enabled, nothing rendered yet)
        if (const int rc = kzFilmResolve(scene, film, ds->lastStream)) return rc;
        HIP_TRY(hipStreamSynchronize(ds->lastStream));
    }
    HIP_TRY(hipMemcpy(out, film.texels, nFloats * sizeof(float), hipMemcpyDeviceToHost));
    return KZ_OK;
}
int kz_film_download_on(KzScene *scene, int device, float *film, size_t nFloats) {
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    return downloadFilm(scene, ds, ds->picture(), true, film, nFloats);
}
int kz_film_download(KzScene *scene, float *film, size_t nFloats) { return kz_film_download_on(scene, -1, film, nFloats); }

// ---- the entry points of include/kazen_mi355x_aov.h that only touch replica state (kz_aov_samples is kz_render.hip's) ----
int kz_scene_set_aovs(KzScene *scene, uint32_t mask) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "null scene");
    if (mask & ~KZ_AOV_ALL) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_aovs: mask %u has bits outside KZ_AOV_ALL (%u)", mask, KZ_AOV_ALL);
    KzReplicaSet *rs = replicaSet(scene);
    std::vector<KzDeviceState *> v;
    if (rs) { std::lock_guard<std::mutex> g(rs->m); v = rs->v; }
    for (KzDeviceState *ds : v) {                                      // queued work finishes with the sums it was launched with
        HIP_TRY(hipSetDevice(ds->hipDevice));
        HIP_TRY(hipDeviceSynchronize());
        for (int f = 0; f < 3; ++f) if (scene->aovMask & ~mask & (1u << f)) ds->aov(f).free();
    }
    scene->aovMask = mask;
    return KZ_OK;
}
int kz_scene_aovs(const KzScene *scene, uint32_t *mask) {
    if (!scene || !mask) return kz_fail(KZ_ERR_INVALID_ARG, "null argument");
    *mask = scene->aovMask;
    return KZ_OK;
}
int kz_aov_download_on(KzScene *scene, int device, uint32_t aov, float *film, size_t nFloats) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "null scene");
    if ((aov != KZ_AOV_ALBEDO && aov != KZ_AOV_NORMAL && aov != KZ_AOV_DEPTH) || !(scene->aovMask & aov))
        return kz_fail(KZ_ERR_INVALID_ARG, "kz_aov_download: aov %u must be exactly one enabled AOV bit (the scene's mask is %u)", aov, scene->aovMask);
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    return downloadFilm(scene, ds, ds->aov(aov == KZ_AOV_ALBEDO ? 0 : (aov == KZ_AOV_NORMAL ? 1 : 2)), false, film, nFloats);
}
int kz_aov_download(KzScene *scene, uint32_t aov, float *film, size_t nFloats) { return kz_aov_download_on(scene, -1, aov, film, nFloats); }

int kz_aov_info(KzScene *scene, int device, uint64_t *bytes) {
    KzDeviceState *ds; int rc;
    if (!bytes) return kz_fail(KZ_ERR_INVALID_ARG, "null bytes");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    *bytes = ds->aovBytes();
    return KZ_OK;
}

// ---- the entry points of include/kazen_mi355x_variance.h that only touch replica state (kz_denoise_variance* are kz_denoise.hip's) ----
int kz_scene_set_variance(KzScene *scene, int32_t mode) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_variance: null scene");
    if (mode < 0 || mode > KZ_VARIANCE_ONE_PASS) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_set_variance: mode %d (0 = off, 1 = on, 2 = on with two tap launches, 3 = on with the one-pass tap kernel)", mode);
    KzReplicaSet *rs = replicaSet(scene);
    std::vector<KzDeviceState *> v;
    if (rs) { std::lock_guard<std::mutex> g(rs->m); v = rs->v; }
    for (KzDeviceState *ds : v) {                                      // queued work finishes with the sums it was launched with
        HIP_TRY(hipSetDevice(ds->hipDevice));
        HIP_TRY(hipDeviceSynchronize());
        if (!mode) { ds->moment().free(); ds->momentSamples = 0; }
    }
    scene->varianceMode = mode;
    return KZ_OK;
}
int kz_scene_variance(const KzScene *scene, int32_t *mode) {
    if (!scene || !mode) return kz_fail(KZ_ERR_INVALID_ARG, "kz_scene_variance: null argument");
    *mode = scene->varianceMode;
    return KZ_OK;
}
int kz_variance_download(KzScene *scene, int device, float *film, size_t nFloats) {
    if (!scene) return kz_fail(KZ_ERR_INVALID_ARG, "kz_variance_download: null scene");
    if (!scene->varianceMode) return kz_fail(KZ_ERR_STATE, "kz_variance_download: the second-moment film is switched off (kz_scene_set_variance)");
    KzDeviceState *ds; int rc;
    if ((rc = findReplica(scene, device, &ds))) return rc;
    return downloadFilm(scene, ds, ds->moment(), false, film, nFloats);
}
int kz_variance_info(KzScene *scene, int device, uint64_t *bytes, uint32_t *samples) {
    KzDeviceState *ds; int rc;
    if (!bytes && !samples) return kz_fail(KZ_ERR_INVALID_ARG, "kz_variance_info: null bytes and samples");
    if ((rc = findReplica(scene, device, &ds))) return rc;
    if (bytes) *bytes = ds->moment().bytes();
    if (samples) *samples = ds->momentSamples;
    return KZ_OK;
}

// ImageBlock::toBitmap (block.cpp:39-45) + Bitmap::savePNG's tone map (bitmap.cpp:45-52): the film is resolved to the 8-bit
// sRGB raster on the device, so the host link carries 3 bytes per pixel instead of the 16-byte film texel.
int kz_film_to_srgb8(KzScene *scene, uint8_t *rgb8, size_t nBytes) {
    KzDeviceState *ds; int rc;
    if ((rc = requireDevice(scene, &ds))) return rc;
    return kzFilmSrgb8(scene, ds, ds->picture().texels, rgb8, nBytes);
}

} // extern "C"

// kz_film_srgb8 of a film-shaped buffer of the replica (its film, or the denoiser's result: kz_denoise.hip), behind the work queued on ds->lastStream
int kzFilmSrgb8(KzScene *scene, KzDeviceState *ds, const float4 *film, uint8_t *rgb8, size_t nBytes) {
    int rc;
    const KzParams &P = scene->prm;
    const size_t need = (size_t)P.width * (size_t)P.height * 3;
    if (!rgb8 || nBytes != need) return kz_fail(KZ_ERR_INVALID_ARG, "rgb8 buffer must hold %zu bytes", need);
    if (!ds->srgb && (rc = ds->srgb.alloc(need))) return rc;                        // staging raster kept with the replica
    const uint32_t n = (uint32_t)(P.width * P.height);
    hipLaunchKernelGGL(kz_film_srgb8, dim3((n + 255) / 256), dim3(256), 0, ds->lastStream, film, P.width, P.height, P.border, ds->srgb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ds->lastStream));
    HIP_TRY(hipMemcpy(rgb8, ds->srgb, need, hipMemcpyDeviceToHost));
    return KZ_OK;
}

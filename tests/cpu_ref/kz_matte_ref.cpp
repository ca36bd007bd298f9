// kz_matte_ref.cpp - TEST-ONLY CPU reference of the ID mattes (include_ext/kazen_mi355x_matte.h): the key of every sample from the oracle's own first-hit path - this
// translation unit includes oracle/kz_oracle.cpp unchanged and reuses its Sampler, camera and rayIntersect, exactly as tests/cpu_ref/kz_aov_ref.cpp does - and the
// table rule, rank, layer and top in plain sequential C++. Never linked into the product; tests/test_matte_cpu.py compiles it with the oracle's flags.
//
// The scene is created by kzo_scene_create with the path_mis tag (the oracle refuses every other one); the integrator is the argument of the entry points: it
// decides one thing only, whether a first hit on an invisible light is walked through (path_mis) or kept (normals, ao, path_mats).
#include "../../oracle/kz_oracle.cpp"
#include "../../include_ext/kazen_mi355x_matte.h"

#include <algorithm>

namespace kzo {

struct MatteKeys { uint32_t mesh, bsdf; bool hit; };

// the first hit the integrator shades (kz_aov_ref.cpp featuresOf): its mesh and that mesh's BSDF row - a mesh without one has the default diffuse, which the
// library keeps in the row behind the description's rows
static MatteKeys matteKeysOf(const Scene &sc, int integ, const Ray &ray, LocalStats &ls) {
    MatteKeys k; k.mesh = 0; k.bsdf = 0; k.hit = false;
    Intersection its;
    if (!rayIntersect(sc, ray, its, false, ls)) return k;
    if (integ == KZ_INTEGRATOR_PATH_MIS && sc.meshes[its.mesh].light >= 0 && !sc.lights[sc.meshes[its.mesh].light].primaryVisibility) {
        Ray newRay(its.p + sc.integ.traceBias * ray.d, ray.d);                     // integrator.cpp:214-219 (H6): the result is ignored on a miss
        rayIntersect(sc, newRay, its, false, ls);
    }
    const int b = sc.meshes[its.mesh].bsdf;
    k.mesh = (uint32_t)its.mesh; k.bsdf = b < 0 ? (uint32_t)sc.bsdfs.size() : (uint32_t)b; k.hit = true;
    return k;
}

static MatteKeys matteSample(const Scene &sc, int integ, Sampler &sampler, int px, int py, uint32_t j, LocalStats &ls) {
    sampler.generateSample(px, py, j);
    float jx, jy; sampler.nextPixel2D(jx, jy);
    float ax, ay; sampler.next2D(ax, ay);
    Ray ray; cameraSampleRay(sc, (float)px + jx, (float)py + jy, ax, ay, ray);
    return matteKeysOf(sc, integ, ray, ls);
}

// THE RULE for one sample, written as the header states it
static void matteCount(KzMatteTexel &t, bool hit, uint32_t key) {
    if (!hit) { t.miss += 1; return; }
    for (int k = 0; k < KZ_MATTE_SLOTS; ++k) if (t.count[k] > 0 && t.id[k] == key) { t.count[k] += 1; return; }      // a key that already has a slot
    for (int k = 0; k < KZ_MATTE_SLOTS; ++k) if (t.count[k] == 0) { t.id[k] = key; t.count[k] = 1; return; }          // the lowest free slot
    t.other += 1;                                                                                                     // every slot is taken
}

} // namespace kzo

extern "C" {

// 3 words per sample: mesh | bsdf row | hit (0 / 1; a miss has mesh = bsdf = 0)
void kzm_samples(void *s, int integ, uint32_t n, const int32_t *pxy, const uint32_t *idx, uint32_t *out) { kzo::FtzScope ftz_;
    using namespace kzo;
    Scene &sc = *(Scene *)s; Sampler sm; sm.sc = &sc; sm.type = sc.smp.type; LocalStats ls;
    for (uint32_t i = 0; i < n; ++i) {
        const MatteKeys k = matteSample(sc, integ, sm, pxy[2 * i], pxy[2 * i + 1], idx[i], ls);
        out[3 * (size_t)i] = k.mesh; out[3 * (size_t)i + 1] = k.bsdf; out[3 * (size_t)i + 2] = k.hit ? 1u : 0u;
    }
}

// The table of `key` (KZ_MATTE_MESH / KZ_MATTE_BSDF) over the rendered samples [s0, s1) of the pixels of the rectangle [x0, x0 + w) x [y0, y0 + h), counted on top
// of what `table` (width x height records, row-major) holds: pixel by pixel, ascending sample index.
int kzm_table(void *s, int integ, uint32_t key, uint32_t s0, uint32_t s1, int x0, int y0, int w, int h, KzMatteTexel *table) { kzo::FtzScope ftz_;
    using namespace kzo;
    Scene *scp = (Scene *)s; if (!scp || !table || (key != KZ_MATTE_MESH && key != KZ_MATTE_BSDF)) return KZ_ERR_INVALID_ARG;
    Scene &sc = *scp; Sampler sm; sm.sc = &sc; sm.type = sc.smp.type; LocalStats ls;
    if (x0 < 0 || y0 < 0 || x0 + w > sc.cam.width || y0 + h > sc.cam.height) return KZ_ERR_INVALID_ARG;
    for (int py = y0; py < y0 + h; ++py)
        for (int px = x0; px < x0 + w; ++px)
            for (uint32_t j = s0; j < s1; ++j) {
                const MatteKeys k = matteSample(sc, integ, sm, px, py, j, ls);
                matteCount(table[(size_t)py * sc.cam.width + px], k.hit, key == KZ_MATTE_MESH ? k.mesh : k.bsdf);
            }
    return KZ_OK;
}

// The same rule over caller-supplied keys: nPix x S words, pixel-major, KZ_MATTE_NONE = a miss; record p starts from tables[p]
void kzm_accumulate(const uint32_t *keys, uint32_t nPix, uint32_t S, KzMatteTexel *tables) {
    for (uint32_t p = 0; p < nPix; ++p)
        for (uint32_t j = 0; j < S; ++j) { const uint32_t k = keys[(size_t)p * S + j]; kzo::matteCount(tables[p], k != KZ_MATTE_NONE, k); }
}

// rank: count descending, ties to the lower id, free slots last
void kzm_rank(const KzMatteTexel *in, size_t n, KzMatteTexel *out) {
    for (size_t i = 0; i < n; ++i) {
        std::pair<uint32_t, uint32_t> e[KZ_MATTE_SLOTS];          // (count, id)
        for (int k = 0; k < KZ_MATTE_SLOTS; ++k) e[k] = {in[i].count[k], in[i].id[k]};
        std::stable_sort(e, e + KZ_MATTE_SLOTS, [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) { return a.first > b.first || (a.first == b.first && a.second < b.second); });
        out[i] = in[i];
        for (int k = 0; k < KZ_MATTE_SLOTS; ++k) { out[i].count[k] = e[k].first; out[i].id[k] = e[k].second; }
    }
}

void kzm_layer(const KzMatteTexel *in, size_t n, uint32_t id, float *coverage) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t total = in[i].other + in[i].miss, count = 0;
        for (int k = 0; k < KZ_MATTE_SLOTS; ++k) { total += in[i].count[k]; if (in[i].count[k] > 0 && in[i].id[k] == id) count = in[i].count[k]; }
        coverage[i] = total ? (float)count / (float)total : 0.0f;
    }
}

void kzm_top(const KzMatteTexel *in, size_t n, uint32_t *ids) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t bestCount = 0, bestId = KZ_MATTE_NONE;
        for (int k = 0; k < KZ_MATTE_SLOTS; ++k) {
            const uint32_t c = in[i].count[k], d = in[i].id[k];
            if (c > 0 && (c > bestCount || (c == bestCount && d < bestId))) { bestCount = c; bestId = d; }
        }
        ids[i] = (bestCount == 0 || in[i].miss >= bestCount) ? KZ_MATTE_NONE : bestId;
    }
}

} // extern "C"

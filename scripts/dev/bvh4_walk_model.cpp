// Development tool (host only, no GPU): what a child-order rule of the per-lane BVH4 traversal costs in node packets and triangle tests per ray, priced by a
// scalar walk of the REAL tree - kz_build_bvh and kz_collapse_bvh4 of ../../nano-kazen_amd/csrc/kz_bvh.cpp, linked unchanged.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I nano-kazen_amd/csrc scripts/dev/bvh4_walk_model.cpp nano-kazen_amd/csrc/kz_bvh.cpp -pthread -o bvh4_walk_model
//   bvh4_walk_model <triangles> <rule> [seed=1] [rays=100000] [zmin=-2] [occlusion file]
//
// The scene is the C4 soup in small: <triangles> random triangles in [-1, 1]^3 with edges of +-s (nine uniform draws each: centre, two edge vectors; s = 0.02
// at 10^6 triangles and scaled with the cube root of the count below that, so that a box of the tree overlaps as many neighbours), the closed room
// [-1.2, 1.2]^2 x [-1.2, 3.6] and the eight light quads under its ceiling. Rays start on soup triangles (zmin: only on those whose centre has z >= zmin -
// the layer that faces the camera): closest-hit rays in uniform directions, any-hit rays towards points on the lights with tmin = 1e-3 and
// tmax = distance - 1e-3, as the integrator forms its shadow rays.
//
// The walk follows kz_wf_trace (kz_wavefront.h) and node4KeysOf (kz_devfn.h): the slab test in the FMA form on the quantised boxes with the far side widened by
// 1.0000004, the 1e-20 stand-in for a zero direction component, one child taken next and the other hit children pushed in slot order, no culling at a pop, the
// triangle test of triTestV. Closest-hit rays always take the nearest entry. <rule> is the order of the any-hit rays:
//   nearest         the child with the least max(tnear, tmin); ties to the lower slot        (the closest-hit rule)
//   overlap         the child with the largest f - n, the part of [tmin, tmax] inside its box, compared as the kernel's key: the float's bits without the low
//                   three; ties to the higher slot                                                (kz_wf_trace<4>)
//   overlap-sorted  the same, and the deferred children pushed so that the larger overlap is popped first
//   farthest        the child with the largest exit distance min(tfar, tmax)
//   leaf            a leaf child before an inner one, then nearest
// Prints one line: the tree's size, packets and triangle tests per closest-hit ray and per any-hit ray, and the share of occluded any-hit rays. With an
// occlusion file: one '0' / '1' per any-hit ray - the answers of two rules on the same seed must be the same bytes (tests/test_shadow_order_cpu.py).
#include "kz_internal.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
// pcg32 (O'Neill), one stream
struct Rng {
    uint64_t state, inc;
    explicit Rng(uint64_t seed) : state(0), inc((seed << 1) | 1u) { next(); state += 0x853c49e6748fea9bULL ^ seed; next(); }
    uint32_t next() {
        const uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        const uint32_t x = (uint32_t)(((old >> 18) ^ old) >> 27), r = (uint32_t)(old >> 59);
        return (x >> r) | (x << ((32 - r) & 31));
    }
    float uniform() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
};
struct V { float x, y, z; };
V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
uint32_t bitsOf(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

enum Rule { NEAREST, OVERLAP, OVERLAP_SORTED, FARTHEST, LEAF_FIRST };
struct Tree { std::vector<KzNode4> nodes4; std::vector<KzTri> tris; uint32_t root; };
struct Cost { unsigned long long packets = 0, tests = 0; };

// triTestV of kz_devfn.h on a leaf triangle
bool triTest(const KzTri &k, V o, V d, float tmin, float tmax, float &t) {
    const V p0 = {k.p0[0], k.p0[1], k.p0[2]}, e1 = {k.e1[0], k.e1[1], k.e1[2]}, e2 = {k.e2[0], k.e2[1], k.e2[2]};
    const V pvec = cross(d, e2);
    const float det = dot(e1, pvec);
    if (det > -1e-8f && det < 1e-8f) return false;
    const float inv = 1.0f / det;
    const V tvec = o - p0;
    const float u = dot(tvec, pvec) * inv;
    if (u < 0.0f || u > 1.0f) return false;
    const V qvec = cross(tvec, e1);
    const float v = dot(d, qvec) * inv;
    if (v < 0.0f || u + v > 1.0f) return false;
    t = dot(e2, qvec) * inv;
    return t >= tmin && t <= tmax;
}
// node4KeysOf: the clamped entry and exit distance of the four children; hit[i] = n <= f
void slabs(const KzNode4 &nd, V o, float rx, float ry, float rz, float tmin, float tmax, float (&n)[4], float (&f)[4], bool (&hit)[4]) {
    const float ax = nd.scaleX * rx, ay = nd.scaleY * ry, az = nd.scaleZ * rz;
    const float bx = (nd.p[0] - o.x) * rx, by = (nd.p[1] - o.y) * ry, bz = (nd.p[2] - o.z) * rz;
    const uint32_t nX = rx >= 0.f ? nd.qlo[0] : nd.qhi[0], fX = rx >= 0.f ? nd.qhi[0] : nd.qlo[0];
    const uint32_t nY = ry >= 0.f ? nd.qlo[1] : nd.qhi[1], fY = ry >= 0.f ? nd.qhi[1] : nd.qlo[1];
    const uint32_t nZ = rz >= 0.f ? nd.qlo[2] : nd.qhi[2], fZ = rz >= 0.f ? nd.qhi[2] : nd.qlo[2];
    for (int i = 0; i < 4; ++i) {
        const float nx = std::fmaf((float)((nX >> (8 * i)) & 0xffu), ax, bx), fx = std::fmaf((float)((fX >> (8 * i)) & 0xffu), ax, bx);
        const float ny = std::fmaf((float)((nY >> (8 * i)) & 0xffu), ay, by), fy = std::fmaf((float)((fY >> (8 * i)) & 0xffu), ay, by);
        const float nz = std::fmaf((float)((nZ >> (8 * i)) & 0xffu), az, bz), fz = std::fmaf((float)((fZ >> (8 * i)) & 0xffu), az, bz);
        n[i] = std::fmax(std::fmax(std::fmax(nx, ny), nz), tmin);
        f[i] = std::fmin(std::fmin(std::fmin(fx, fy), fz) * 1.0000004f, tmax);
        hit[i] = n[i] <= f[i];
    }
}
float rcpOf(float d) { return 1.0f / (std::fabs(d) < 1e-20f ? std::copysign(1e-20f, d) : d); }

// one ray; anyHit: stops at the first triangle on the segment. Returns whether something was hit.
bool walk(const Tree &T, V o, V d, float tmin, float tmax, bool anyHit, Rule rule, Cost &c) {
    if (T.root == 0xFFFFFFFFu) return false;
    const float rx = rcpOf(d.x), ry = rcpOf(d.y), rz = rcpOf(d.z);
    std::vector<uint32_t> stack;
    uint32_t cur = T.root;
    bool found = false;
    for (;;) {
        if (cur & 0x80000000u) {
            const uint32_t start = (cur & 0x7fffffffu) >> 3, count = (cur & 7u) + 1;
            for (uint32_t i = 0; i < count; ++i) {
                float t;
                c.tests++;
                if (!triTest(T.tris[start + i], o, d, tmin, tmax, t)) continue;
                if (anyHit) return true;
                found = true; tmax = t;
            }
        } else {
            c.packets++;
            const KzNode4 &nd = T.nodes4[cur];
            float n[4], f[4]; bool hit[4];
            slabs(nd, o, rx, ry, rz, tmin, tmax, n, f, hit);
            // the key of every hit child; the child with the LEAST key is taken next
            uint64_t key[4]; int best = -1;
            const Rule r = anyHit ? rule : NEAREST;
            for (int i = 0; i < 4; ++i) {
                if (!hit[i]) continue;
                if (r == NEAREST) key[i] = (uint64_t)((bitsOf(n[i]) & ~3u) | (uint32_t)i);
                else if (r == LEAF_FIRST) key[i] = ((uint64_t)(nd.child[i] & 0x80000000u ? 0 : 1) << 32) | ((bitsOf(n[i]) & ~3u) | (uint32_t)i);
                else if (r == FARTHEST) key[i] = 0xFFFFFFFFull - ((bitsOf(f[i]) & ~3u) | (uint32_t)i);
                else key[i] = 0xFFFFFFFFull - ((bitsOf(f[i] - n[i]) & ~7u) | (4u + (uint32_t)i));
                if (best < 0 || key[i] < key[best]) best = i;
            }
            if (best >= 0) {
                int rest[3], nr = 0;
                for (int i = 0; i < 4; ++i) if (hit[i] && i != best) rest[nr++] = i;
                if (r == OVERLAP_SORTED)          // pushed in descending key order: the least key (largest overlap) is popped first
                    for (int a = 0; a < nr; ++a) for (int b = a + 1; b < nr; ++b) if (key[rest[b]] > key[rest[a]]) { const int t = rest[a]; rest[a] = rest[b]; rest[b] = t; }
                for (int a = 0; a < nr; ++a) stack.push_back(nd.child[rest[a]]);
                cur = nd.child[best];
                continue;
            }
        }
        if (stack.empty()) return found;
        cur = stack.back(); stack.pop_back();
    }
}

void addTri(std::vector<KzBuildTri> &bt, V a, V b, V c, uint32_t mesh) {
    KzBuildTri t;
    const V v[3] = {a, b, c};
    for (int k = 0; k < 3; ++k) { t.v[k][0] = v[k].x; t.v[k][1] = v[k].y; t.v[k][2] = v[k].z; }
    t.mesh = mesh; t.prim = (uint32_t)bt.size(); t.gid = (uint32_t)bt.size();
    bt.push_back(t);
}
void addQuad(std::vector<KzBuildTri> &bt, V a, V b, V c, V d, uint32_t mesh) { addTri(bt, a, b, c, mesh); addTri(bt, a, c, d, mesh); }
}

int main(int argc, char **argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <triangles> nearest|overlap|overlap-sorted|farthest|leaf [seed=1] [rays=100000] [zmin=-2] [occlusion file]\n", argv[0]); return 2; }
    const uint32_t nTris = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    const std::string rn = argv[2];
    Rule rule;
    if (rn == "nearest") rule = NEAREST; else if (rn == "overlap") rule = OVERLAP; else if (rn == "overlap-sorted") rule = OVERLAP_SORTED;
    else if (rn == "farthest") rule = FARTHEST; else if (rn == "leaf") rule = LEAF_FIRST; else { std::fprintf(stderr, "unknown rule %s\n", rn.c_str()); return 2; }
    const uint64_t seed = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 1;
    const uint32_t nRays = argc > 4 ? (uint32_t)std::strtoul(argv[4], nullptr, 10) : 100000u;
    const float zmin = argc > 5 ? (float)std::atof(argv[5]) : -2.f;
    const char *occPath = argc > 6 ? argv[6] : nullptr;

    // ---- the scene
    std::vector<KzBuildTri> bt;
    Rng rs(seed);
    const float s = 0.02f * std::cbrt(1.0e6f / (float)(nTris ? nTris : 1));
    for (uint32_t i = 0; i < nTris; ++i) {
        float u[9];
        for (float &x : u) x = rs.uniform();
        const V c = {2 * u[0] - 1, 2 * u[1] - 1, 2 * u[2] - 1};
        addTri(bt, c, {c.x + s * (2 * u[3] - 1), c.y + s * (2 * u[4] - 1), c.z + s * (2 * u[5] - 1)}, {c.x + s * (2 * u[6] - 1), c.y + s * (2 * u[7] - 1), c.z + s * (2 * u[8] - 1)}, i % 8);
    }
    const float x0 = -1.2f, x1 = 1.2f, y0 = -1.2f, y1 = 1.2f, z0 = -1.2f, z1 = 3.6f;
    addQuad(bt, {x0, y0, z0}, {x1, y0, z0}, {x1, y0, z1}, {x0, y0, z1}, 8); addQuad(bt, {x0, y1, z0}, {x1, y1, z0}, {x1, y1, z1}, {x0, y1, z1}, 8);
    addQuad(bt, {x0, y0, z0}, {x0, y1, z0}, {x0, y1, z1}, {x0, y0, z1}, 8); addQuad(bt, {x1, y0, z0}, {x1, y1, z0}, {x1, y1, z1}, {x1, y0, z1}, 8);
    addQuad(bt, {x0, y0, z0}, {x1, y0, z0}, {x1, y1, z0}, {x0, y1, z0}, 8); addQuad(bt, {x0, y0, z1}, {x1, y0, z1}, {x1, y1, z1}, {x0, y1, z1}, 8);
    struct Light { float cx, cz; } lights[8];
    { int k = 0; const float h = 0.2f;
      for (float cx : {-0.75f, -0.25f, 0.25f, 0.75f}) for (float cz : {0.0f, 2.3f}) {
          lights[k] = {cx, cz};
          addQuad(bt, {cx - h, 1.19f, cz - h}, {cx - h, 1.19f, cz + h}, {cx + h, 1.19f, cz + h}, {cx + h, 1.19f, cz - h}, 9 + (uint32_t)k); ++k; } }

    Tree T;
    std::vector<KzNode> nodes; KzBvhInfo info; std::string err;
    uint32_t rootRef = 0xFFFFFFFFu; int stackBound = 1;
    std::memset(&info, 0, sizeof info);
    if (kz_build_bvh(bt, nodes, T.tris, rootRef, info, err) != KZ_OK) { std::fprintf(stderr, "kz_build_bvh: %s\n", err.c_str()); return 1; }
    if (kz_collapse_bvh4(nodes, rootRef, T.nodes4, T.root, stackBound) != KZ_OK) { std::fprintf(stderr, "kz_collapse_bvh4 failed\n"); return 1; }

    // ---- the rays: origins on soup triangles (of the layer z >= zmin)
    std::vector<uint32_t> pool;
    for (uint32_t i = 0; i < nTris; ++i) if (bt[i].v[0][2] >= zmin) pool.push_back(i);
    if (pool.empty()) { std::fprintf(stderr, "no soup triangle with z >= %g\n", zmin); return 1; }
    Rng rr(seed + 1000003u);
    Cost closest, any;
    unsigned long long occluded = 0, closestHits = 0;
    std::string occ;
    for (uint32_t r = 0; r < nRays; ++r) {
        const KzBuildTri &t = bt[pool[rr.next() % pool.size()]];
        float a = rr.uniform(), b = rr.uniform();
        if (a + b > 1) { a = 1 - a; b = 1 - b; }
        const V o = {t.v[0][0] + a * (t.v[1][0] - t.v[0][0]) + b * (t.v[2][0] - t.v[0][0]), t.v[0][1] + a * (t.v[1][1] - t.v[0][1]) + b * (t.v[2][1] - t.v[0][1]),
                     t.v[0][2] + a * (t.v[1][2] - t.v[0][2]) + b * (t.v[2][2] - t.v[0][2])};
        // closest hit: a uniform direction
        const float cz = 2 * rr.uniform() - 1, ph = 6.2831853f * rr.uniform(), sr = std::sqrt(std::fmax(0.f, 1 - cz * cz));
        closestHits += walk(T, o, {sr * std::cos(ph), sr * std::sin(ph), cz}, 1e-3f, INFINITY, false, rule, closest) ? 1 : 0;
        // any hit: towards a point on a light
        const Light &L = lights[rr.next() & 7u];
        const V p = {L.cx + 0.2f * (2 * rr.uniform() - 1), 1.19f, L.cz + 0.2f * (2 * rr.uniform() - 1)};
        const V v = p - o;
        const float dist = std::sqrt(dot(v, v));
        const bool hit = walk(T, o, {v.x / dist, v.y / dist, v.z / dist}, 1e-3f, dist - 1e-3f, true, rule, any);
        occluded += hit ? 1 : 0;
        if (occPath) occ.push_back(hit ? '1' : '0');
    }
    if (occPath) {
        FILE *fo = std::fopen(occPath, "wb");
        if (!fo || std::fwrite(occ.data(), 1, occ.size(), fo) != occ.size()) { std::fprintf(stderr, "cannot write %s\n", occPath); return 1; }
        std::fclose(fo);
    }
    const double n = nRays ? (double)nRays : 1.0;
    std::printf("{\"triangles\": %u, \"rule\": \"%s\", \"seed\": %llu, \"rays\": %u, \"packets4\": %zu, \"leafTriangles\": %zu, \"stackBound\": %d, "
                "\"closest\": {\"packets\": %.4f, \"tests\": %.4f, \"hit\": %.4f}, \"anyhit\": {\"packets\": %.4f, \"tests\": %.4f, \"occluded\": %.4f}}\n",
                nTris, rn.c_str(), (unsigned long long)seed, nRays, T.nodes4.size(), T.tris.size(), stackBound,
                closest.packets / n, closest.tests / n, closestHits / n, any.packets / n, any.tests / n, occluded / n);
    return 0;
}

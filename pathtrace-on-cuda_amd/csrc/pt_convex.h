// pt_convex.h — what the convex-region queries share (pt_convex.hip: pt_convex_count, pt_convex_any, pt_convex_list; include/pt_api.h:
// "Convex-region queries"): the ONE statement of the float32 class key h(Q, k) of a region Q — the intersection of
// m <= 8 half-spaces s_j(x) <= d_j, s_j(x) = (n.x*x.x + n.y*x.y) + n.z*x.z — and a primitive k — 0 inside, 1 touching, +inf no member —,
// and the walk over either tree that hands every primitive below a node the region may reach to a query's sink.
//
// Why the walk is exact: rule 1 of h is a floor — a member has, for every plane, a vertex v with s_j(v) <= d_j.  The walk culls a node
// box (lo, hi) when for some j !(s_j(p) <= d_j) at the corner p of the box that minimises s_j: per axis lo where n >= 0, hi otherwise.
// Rounding to nearest is monotone: fl(n * x) is monotone in x (non-decreasing for n >= 0, non-increasing otherwise), fl(u + v) is
// monotone in each addend, so s_j(p) <= s_j(v) in FLOAT32 for every float point v of the box — the same three products and two sums,
// no real-number slack.  The vertices a, b = a + E1, c = a + E2 of a record lie in the record's box, and every widened box of either
// tree contains the boxes of the records below it (section 29): a culled node holds no member.  A NaN in a plane makes every test
// false: every node is culled and every key is +inf, consistently.  Nothing is ordered, a stack entry is a bare ref, and no popped
// entry is tested again: the shape of pt_box.h's walks.
//
// Registers: a lane's planes are eight float4 in VGPRs.  Every loop over planes is fully unrolled to kConvexPlanes under the guard
// j < m, m a kernel argument: the index is a constant after unrolling (no scratch) and the guard a scalar branch.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_nearest.h"
#include "pt_box.h"

namespace ptd {

constexpr int kConvexPlanes = 8;      // PT_CONVEX_MAX_PLANES

// h(Q, triangle) of the header, operation for operation: pl = the m PLANE4 records n.xyz | d of the region.  Self-contained (no helper of
// pt_math.h), so that tools/convex_host.cpp compiles this text for the host and tests/test_convex_queries.py holds it to numpy bit for bit.
PT_DEV float convex_tri_key(const float4* pl, int m, const f3& a, const f3& ab, const f3& ac)
{
    const float kInf = __builtin_inff();
    const float bx = a.x + ab.x, by = a.y + ab.y, bz = a.z + ab.z, cx = a.x + ac.x, cy = a.y + ac.y, cz = a.z + ac.z;
    bool valid = true, none = false, all = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j < m) {
            const float4 n = pl[j];
            valid &= (__builtin_fabsf(n.x) < kInf) & (__builtin_fabsf(n.y) < kInf) & (__builtin_fabsf(n.z) < kInf);      // finite: no NaN, no inf
            const bool ia = (n.x * a.x + n.y * a.y) + n.z * a.z <= n.w;
            const bool ib = (n.x * bx + n.y * by) + n.z * bz <= n.w;
            const bool ic = (n.x * cx + n.y * cy) + n.z * cz <= n.w;
            none |= !(ia | ib | ic);      // the floor: a plane with every vertex outside
            all &= ia & ib & ic;
        }
    }
    if (!valid | none) return kInf;
    return all ? 0.f : 1.f;
}

// h(Q, sphere) of the header: s = center.xyz | rad; membership refers to the sphere's surface
PT_DEV float convex_sphere_key(const float4* pl, int m, const float4& s)
{
    const float kInf = __builtin_inff();
    bool valid = true, none = false, all = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j < m) {
            const float4 n = pl[j];
            valid &= (__builtin_fabsf(n.x) < kInf) & (__builtin_fabsf(n.y) < kInf) & (__builtin_fabsf(n.z) < kInf);
            const float len = __builtin_sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
            const float r = s.w * len;
            const float sc = (n.x * s.x + n.y * s.y) + n.z * s.z;
            none |= !(sc - r <= n.w);
            all &= (sc + r <= n.w);
        }
    }
    if (!valid | none) return kInf;
    return all ? 0.f : 1.f;
}

// The floor against a node's box: may anything below the box (clo, chi) be a member?  Per plane the corner that minimises s_j, with
// s_j's own three products and two sums.
PT_DEV bool convex_overlaps(const f3& clo, const f3& chi, const float4* pl, int m)
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j < m) {
            const float4 n = pl[j];
            const float px = n.x >= 0.f ? clo.x : chi.x, py = n.y >= 0.f ? clo.y : chi.y, pz = n.z >= 0.f ? clo.z : chi.z;
            ok &= ((n.x * px + n.y * py) + n.z * pz <= n.w);
        }
    }
    return ok;
}

// The `cnt` triangles at tree position `first` (a leaf of either tree: ~ref = first << 3 | cnt), as box_leaf
template <class SINK>
PT_DEV void convex_leaf(const DevScene& sc, int ref, const float4* pl, int m, SINK& s)
{
    const int code = ~ref, first = code >> 3, cnt = code & 7;
    for (int k = 0; k < cnt; k++) {
        const float4* rec = sc.tri + 3 * (size_t)(first + k);
        const float4 a = rec[0], b = rec[1], c = rec[2];
        box_offer(s, convex_tri_key(pl, m, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z)), __float_as_int(a.w));
    }
}

// The walk over the 4-wide quantised tree, box_walk_quad with the region's node test: at most 3 entries per level (the caller has
// checked 3 * quad_depth + 2 <= kQueryStack), an empty slot recognised by its ref, entry e of a lane's stack at stack[e * 64].
template <class SINK>
PT_DEV void convex_walk_quad(const DevScene& sc, const float4* pl, int m, int* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        if (cur >= 0) {
            const uint4* np = sc.quad + 4 * (size_t)cur;
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const int ref[4] = {(int)n1.x, (int)n1.y, (int)n1.z, (int)n1.w};
            bool have = false;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                f3 clo, chi;
                near_quad_child_box(n0, n2, n3, k, clo, chi);
                if ((ref[k] == -1) | !convex_overlaps(clo, chi, pl, m)) continue;
                if (have) { stack[sp * 64] = ref[k]; sp++; }
                else { cur = ref[k]; have = true; }
            }
            if (have) continue;
        } else {
            convex_leaf(sc, cur, pl, m, s);
            if constexpr (SINK::kStops) { if (s.done()) return; }
        }
        if (sp == 0) return;
        sp--;
        cur = stack[sp * 64];
    }
}

// The walk over the binary tree, box_walk_binary with the region's node test: at most depth - 1 <= 31 entries
template <class SINK>
PT_DEV void convex_walk_binary(const DevScene& sc, const float4* pl, int m, int* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        if constexpr (SINK::kStops) { if (s.done()) return; }
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        f3 loL(q0.x, q0.y, q0.z), hiL(q0.w, q1.x, q1.y), loR(q1.z, q1.w, q2.x), hiR(q2.y, q2.z, q2.w);
        widen_binary(loL, hiL);
        widen_binary(loR, hiR);
        const bool inL = convex_overlaps(loL, hiL, pl, m), inR = convex_overlaps(loR, hiR, pl, m);
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        if (refL < 0 && inL) convex_leaf(sc, refL, pl, m, s);
        if (refR < 0 && inR) convex_leaf(sc, refR, pl, m, s);
        const bool okL = (refL >= 0) & inL, okR = (refR >= 0) & inR;
        if (okL & okR) {
            stack[sp * 64] = refR;
            sp++;
            cur = refL;
        } else if (okL) {
            cur = refL;
        } else if (okR) {
            cur = refR;
        } else {
            if (sp == 0) return;
            sp--;
            cur = stack[sp * 64];
        }
    }
}

// Region pl[0 .. m): the walk, then the spheres in order
template <bool QUAD, class SINK>
PT_DEV void convex_query(const DevScene& sc, const float4* pl, int m, int* stack, SINK& s)
{
    if (QUAD) convex_walk_quad(sc, pl, m, stack, s);
    else convex_walk_binary(sc, pl, m, stack, s);
    for (int j = 0; j < sc.n_spheres; j++) box_offer(s, convex_sphere_key(pl, m, sc.spheres[4 * j]), sc.n_tris + j);
}

}  // namespace ptd

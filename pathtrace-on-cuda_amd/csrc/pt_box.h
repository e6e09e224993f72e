// pt_box.h — what the box queries share (pt_box.hip: pt_box_count, pt_box_any, pt_box_list; include/pt_api.h: "Box queries"; DESIGN.md
// section 41): the ONE statement of the float32 class key g(Q, k) of a box Q and a primitive k — 0 inside, 1 touching, +inf no member —
// and the walk over either tree that hands every primitive below an overlapping leaf to a query's sink.
//
// Why the walk is exact: step 2 of g is a floor, as the last line of f is for the distance queries — a member's record box overlaps Q,
// compared with no rounding in between; every widened child box above it contains that record box (section 29); so a child whose
// widened box fails the SAME per-axis overlap test against Q holds no member.  Nothing is ordered (a node test has no distance), a stack
// entry is a bare ref, and no popped entry is tested again.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_nearest.h"

namespace ptd {

// g(Q, triangle) of the header, operation for operation.  Self-contained (no helper of pt_math.h: dot and cross are written out in
// their order), so that tools/box_host.cpp compiles this text for the host and tests/test_box_queries.py holds it to numpy bit for bit.
PT_DEV float box_tri_key(const f3& lo, const f3& hi, const f3& a, const f3& ab, const f3& ac)
{
    const float kNone = __builtin_inff();
    if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) return kNone;      // an inverted box, any NaN
    const float bx = a.x + ab.x, by = a.y + ab.y, bz = a.z + ab.z, cx = a.x + ac.x, cy = a.y + ac.y, cz = a.z + ac.z;
    const float tlox = __builtin_fminf(__builtin_fminf(a.x, bx), cx), tloy = __builtin_fminf(__builtin_fminf(a.y, by), cy),
                tloz = __builtin_fminf(__builtin_fminf(a.z, bz), cz);
    const float thix = __builtin_fmaxf(__builtin_fmaxf(a.x, bx), cx), thiy = __builtin_fmaxf(__builtin_fmaxf(a.y, by), cy),
                thiz = __builtin_fmaxf(__builtin_fmaxf(a.z, bz), cz);
    if (!(tlox <= hi.x && thix >= lo.x && tloy <= hi.y && thiy >= lo.y && tloz <= hi.z && thiz >= lo.z)) return kNone;      // the floor
    if (tlox >= lo.x && thix <= hi.x && tloy >= lo.y && thiy <= hi.y && tloz >= lo.z && thiz <= hi.z) return 0.f;
    if (__builtin_isinf(lo.x) || __builtin_isinf(lo.y) || __builtin_isinf(lo.z) || __builtin_isinf(hi.x) || __builtin_isinf(hi.y) || __builtin_isinf(hi.z))
        return 1.f;      // a half-space, a slab: the boxes decide (exact); a column infinite on one axis only: conservative
    // the separating axes: the triangle's plane, then edge x axis for the edges ab, ac, bc (the boxes' axes are steps 2 and 3)
    const float ctr[3] = {(lo.x + hi.x) * 0.5f, (lo.y + hi.y) * 0.5f, (lo.z + hi.z) * 0.5f};
    const float h[3] = {__builtin_fmaxf(hi.x - ctr[0], ctr[0] - lo.x), __builtin_fmaxf(hi.y - ctr[1], ctr[1] - lo.y),
                        __builtin_fmaxf(hi.z - ctr[2], ctr[2] - lo.z)};
    const float v[3][3] = {{a.x - ctr[0], a.y - ctr[1], a.z - ctr[2]}, {bx - ctr[0], by - ctr[1], bz - ctr[2]}, {cx - ctr[0], cy - ctr[1], cz - ctr[2]}};
    const float e[3][3] = {{ab.x, ab.y, ab.z}, {ac.x, ac.y, ac.z}, {ac.x - ab.x, ac.y - ab.y, ac.z - ab.z}};
    const float nx = ab.y * ac.z - ab.z * ac.y, ny = -(ab.x * ac.z - ab.z * ac.x), nz = ab.x * ac.y - ab.y * ac.x;
    const float d = (nx * v[0][0] + ny * v[0][1]) + nz * v[0][2];
    const float r = (h[0] * __builtin_fabsf(nx) + h[1] * __builtin_fabsf(ny)) + h[2] * __builtin_fabsf(nz);
    bool sep = __builtin_fabsf(d) > r;
#pragma unroll
    for (int m = 0; m < 3; m++) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int j = (i + 1) % 3, k = (i + 2) % 3;
            const float p0 = v[0][k] * e[m][j] - v[0][j] * e[m][k], p1 = v[1][k] * e[m][j] - v[1][j] * e[m][k],
                        p2 = v[2][k] * e[m][j] - v[2][j] * e[m][k];
            const float rr = h[j] * __builtin_fabsf(e[m][k]) + h[k] * __builtin_fabsf(e[m][j]);
            sep = sep || __builtin_fminf(__builtin_fminf(p0, p1), p2) > rr || __builtin_fmaxf(__builtin_fmaxf(p0, p1), p2) < -rr;
        }
    }
    return sep ? kNone : 1.f;
}

// g(Q, sphere) of the header: s = center.xyz | rad; membership refers to the sphere's surface
PT_DEV float box_sphere_key(const f3& lo, const f3& hi, const float4& s)
{
    const float kNone = __builtin_inff();
    if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) return kNone;
    if (s.x - s.w >= lo.x && s.x + s.w <= hi.x && s.y - s.w >= lo.y && s.y + s.w <= hi.y && s.z - s.w >= lo.z && s.z + s.w <= hi.z) return 0.f;
    const float nx = __builtin_fmaxf(__builtin_fmaxf(lo.x - s.x, s.x - hi.x), 0.f), ny = __builtin_fmaxf(__builtin_fmaxf(lo.y - s.y, s.y - hi.y), 0.f),
                nz = __builtin_fmaxf(__builtin_fmaxf(lo.z - s.z, s.z - hi.z), 0.f);
    const float near2 = (nx * nx + ny * ny) + nz * nz;      // boxdist2(center, lo, hi)
    const float gx = __builtin_fmaxf(__builtin_fabsf(lo.x - s.x), __builtin_fabsf(hi.x - s.x)),
                gy = __builtin_fmaxf(__builtin_fabsf(lo.y - s.y), __builtin_fabsf(hi.y - s.y)),
                gz = __builtin_fmaxf(__builtin_fabsf(lo.z - s.z), __builtin_fabsf(hi.z - s.z));
    const float far2 = (gx * gx + gy * gy) + gz * gz;       // to the farthest corner
    const float rr = s.w * s.w;
    return (near2 <= rr && far2 >= rr) ? 1.f : kNone;
}

// Step 2 of g against a node's box: may anything below the box (clo, chi) be a member of Q = (lo, hi)?
PT_DEV bool box_overlaps(const f3& clo, const f3& chi, const f3& lo, const f3& hi)
{
    return clo.x <= hi.x && chi.x >= lo.x && clo.y <= hi.y && chi.y >= lo.y && clo.z <= hi.z && chi.z >= lo.z;
}

// A candidate goes to a sink as the ray walks hand theirs over (pt_lists.h): wants(), then take() — the two every sink has, the one-slot
// sink included
template <class SINK>
PT_DEV void box_offer(SINK& s, float key, int prim)
{
    if (s.wants(key, prim)) s.take(key, prim);
}

// The `cnt` triangles at tree position `first` (a leaf of either tree: ~ref = first << 3 | cnt), as knear_leaf
template <class SINK>
PT_DEV void box_leaf(const DevScene& sc, int ref, const f3& lo, const f3& hi, SINK& s)
{
    const int code = ~ref, first = code >> 3, cnt = code & 7;
    for (int k = 0; k < cnt; k++) {
        const float4* rec = sc.tri + 3 * (size_t)(first + k);
        const float4 a = rec[0], b = rec[1], c = rec[2];
        box_offer(s, box_tri_key(lo, hi, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z)), __float_as_int(a.w));
    }
}

// The walk over the 4-wide quantised tree, the shape of knear_walk_quad without its keys: a node pushes at most three of its
// overlapping children and descends into the fourth, a leaf pushes nothing — at most 3 entries per level (the caller has checked
// 3 * quad_depth + 2 <= kQueryStack), and the walk ends whatever the floats are, as quad_step's does.  An empty slot's box is inverted,
// not far away: it is recognised by its ref.  Entry e of a lane's stack is stack[e * 64], a bare ref.
template <class SINK>
PT_DEV void box_walk_quad(const DevScene& sc, const f3& lo, const f3& hi, int* stack, SINK& s)
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
                if ((ref[k] == -1) | !box_overlaps(clo, chi, lo, hi)) continue;
                if (have) { stack[sp * 64] = ref[k]; sp++; }
                else { cur = ref[k]; have = true; }
            }
            if (have) continue;
        } else {
            box_leaf(sc, cur, lo, hi, s);
            if constexpr (SINK::kStops) { if (s.done()) return; }
        }
        if (sp == 0) return;
        sp--;
        cur = stack[sp * 64];
    }
}

// The walk over the binary tree, the shape of knear_walk_binary: a leaf child is evaluated on the spot and an entry is pushed only
// where both children are interior and overlap: at most depth - 1 <= 31 entries.
template <class SINK>
PT_DEV void box_walk_binary(const DevScene& sc, const f3& lo, const f3& hi, int* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        if constexpr (SINK::kStops) { if (s.done()) return; }
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        f3 loL(q0.x, q0.y, q0.z), hiL(q0.w, q1.x, q1.y), loR(q1.z, q1.w, q2.x), hiR(q2.y, q2.z, q2.w);
        widen_binary(loL, hiL);
        widen_binary(loR, hiR);
        const bool inL = box_overlaps(loL, hiL, lo, hi), inR = box_overlaps(loR, hiR, lo, hi);
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        if (refL < 0 && inL) box_leaf(sc, refL, lo, hi, s);
        if (refR < 0 && inR) box_leaf(sc, refR, lo, hi, s);
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

// Box (lo, hi): the walk, then the spheres in order
template <bool QUAD, class SINK>
PT_DEV void box_query(const DevScene& sc, const f3& lo, const f3& hi, int* stack, SINK& s)
{
    if (QUAD) box_walk_quad(sc, lo, hi, stack, s);
    else box_walk_binary(sc, lo, hi, stack, s);
    for (int j = 0; j < sc.n_spheres; j++) box_offer(s, box_sphere_key(lo, hi, sc.spheres[4 * j]), sc.n_tris + j);
}

}  // namespace ptd

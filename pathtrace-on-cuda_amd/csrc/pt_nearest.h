// pt_nearest.h — what the distance queries share (pt_nearest.hip: pt_closest_points; pt_knearest.hip: pt_nearest_k, pt_count_within): the
// ONE statement of the float32 function f of include/pt_api.h ("Closest-point queries"), of the box distance their walks prune with,
// of the widening of the child boxes of either tree that the pruning's premise rests on, of the detail record, and the point walk over
// either tree that hands the candidates to a query's sink.  DESIGN.md sections 29, 30 and 38.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"

namespace ptd {

// boxdist2 of the header: squared distance from p to the box, 0 inside.  Every operation is monotone in lo (up) and hi (down) under rounding.
PT_DEV float boxdist2(const f3& p, const f3& lo, const f3& hi)
{
    const float gx = __builtin_fmaxf(__builtin_fmaxf(lo.x - p.x, p.x - hi.x), 0.f);
    const float gy = __builtin_fmaxf(__builtin_fmaxf(lo.y - p.y, p.y - hi.y), 0.f);
    const float gz = __builtin_fmaxf(__builtin_fmaxf(lo.z - p.z, p.z - hi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// seg of the header: squared distance from the point a + q to the segment a .. a + e, t = the clamped parameter (a zero edge: NaN -> 0)
PT_DEV float near_seg(const f3& q, const f3& e, float& t)
{
    t = dot(q, e) / dot(e, e);
    t = (t > 0.f) ? t : 0.f;
    t = (t < 1.f) ? t : 1.f;
    const f3 r = q - t * e;
    return dot(r, r);
}

// f(p, triangle) of the header
PT_DEV float tri_f(const f3& p, const f3& a, const f3& ab, const f3& ac)
{
    const f3 bc = ac - ab, ap = p - a, bp = ap - ab;
    float t;
    const float dEdge = __builtin_fminf(__builtin_fminf(near_seg(ap, ab, t), near_seg(ap, ac, t)), near_seg(bp, bc, t));
    const f3 n = cross(ab, ac);
    const float nn = dot(n, n), h = dot(ap, n);
    const bool inside = nn > 0.f && dot(cross(ab, ap), n) >= 0.f && dot(cross(bc, bp), n) >= 0.f && dot(cross(ap, ac), n) >= 0.f;
    const float dPlane = (h * h) / nn;
    const float dRaw = (inside && dPlane < dEdge) ? dPlane : dEdge;
    const f3 b = a + ab, c = a + ac;
    const f3 lo(__builtin_fminf(__builtin_fminf(a.x, b.x), c.x), __builtin_fminf(__builtin_fminf(a.y, b.y), c.y), __builtin_fminf(__builtin_fminf(a.z, b.z), c.z));
    const f3 hi(__builtin_fmaxf(__builtin_fmaxf(a.x, b.x), c.x), __builtin_fmaxf(__builtin_fmaxf(a.y, b.y), c.y), __builtin_fmaxf(__builtin_fmaxf(a.z, b.z), c.z));
    return __builtin_fmaxf(dRaw, boxdist2(p, lo, hi));
}

PT_DEV float sphere_f(const f3& p, const float4& s)
{
    const f3 pc = p - f3(s.x, s.y, s.z);
    const float g = __builtin_sqrtf(dot(pc, pc)) - s.w;
    return g * g;
}

// The slack of the boxes (DESIGN.md section 29 has the bound): a decoded child box of the 4-wide tree by 2^-20 of |origin| + 255 * scale
// per axis, as quad_order widens its planes; a box of the binary tree by 2^-20 of its larger magnitude per axis.
constexpr float kNearSlack = 9.5367431640625e-7f;      // 2^-20
PT_DEV void widen_binary(f3& lo, f3& hi)
{
    const float sx = __builtin_fmaxf(__builtin_fabsf(lo.x), __builtin_fabsf(hi.x)) * kNearSlack;
    const float sy = __builtin_fmaxf(__builtin_fabsf(lo.y), __builtin_fabsf(hi.y)) * kNearSlack;
    const float sz = __builtin_fmaxf(__builtin_fabsf(lo.z), __builtin_fabsf(hi.z)) * kNearSlack;
    lo = f3(lo.x - sx, lo.y - sy, lo.z - sz);
    hi = f3(hi.x + sx, hi.y + sy, hi.z + sz);
}

// Child k's box of a 4-wide node (n0 .. n3: its four uint4 words, pt_device.h), decoded and widened.  An empty slot's box is
// inverted, not far away: the caller looks at its ref.
PT_DEV void near_quad_child_box(const uint4& n0, const uint4& n2, const uint4& n3, int k, f3& lo, f3& hi)
{
    const f3 org(__uint_as_float(n0.x), __uint_as_float(n0.y), __uint_as_float(n0.z));
    const f3 scl(__uint_as_float(n0.w), __uint_as_float(n3.z), __uint_as_float(n3.w));
    const f3 sl((__builtin_fabsf(org.x) + 255.f * scl.x) * kNearSlack, (__builtin_fabsf(org.y) + 255.f * scl.y) * kNearSlack,
                (__builtin_fabsf(org.z) + 255.f * scl.z) * kNearSlack);
    lo = f3((org.x + scl.x * (float)((n2.x >> (8 * k)) & 0xffu)) - sl.x, (org.y + scl.y * (float)((n2.y >> (8 * k)) & 0xffu)) - sl.y,
            (org.z + scl.z * (float)((n2.z >> (8 * k)) & 0xffu)) - sl.z);
    hi = f3((org.x + scl.x * (float)((n2.w >> (8 * k)) & 0xffu)) + sl.x, (org.y + scl.y * (float)((n3.x >> (8 * k)) & 0xffu)) + sl.y,
            (org.z + scl.z * (float)((n3.y >> (8 * k)) & 0xffu)) + sl.z);
}

// The 8-float detail record of the header for point p and primitive prim (0 <= prim < number of primitives): c.xyz | v | w | side | feature | 0.
// A triangle is read from its surface record (indexed by primitive in the reference's order), which starts with V0 E1 E2, the floats
// its tri record holds.
PT_DEV void near_detail(const DevScene& sc, const float4& q, int prim, float* o)
{
    const f3 p(q.x, q.y, q.z);
    f3 c;
    float v = 0.f, w = 0.f, side, feature;
    if (prim >= sc.n_tris) {
        const float4 s = sc.spheres[4 * (prim - sc.n_tris)];
        const f3 ctr(s.x, s.y, s.z), pc = p - ctr;
        const float l = __builtin_sqrtf(dot(pc, pc));
        c = (l > 0.f) ? ctr + (s.w / l) * pc : f3(ctr.x + s.w, ctr.y, ctr.z);
        side = (l >= s.w) ? 1.f : -1.f;
        feature = 4.f;
    } else {
        const float4* rec = sc.surf + 12 * (size_t)prim;
        const float4 s0 = rec[0], s1 = rec[1], s2 = rec[2];
        const f3 a(s0.x, s0.y, s0.z), ab(s0.w, s1.x, s1.y), ac(s1.z, s1.w, s2.x);
        const f3 bc = ac - ab, ap = p - a, bp = ap - ab;
        float t1, t2, t3;
        const float d1 = near_seg(ap, ab, t1), d2 = near_seg(ap, ac, t2), d3 = near_seg(bp, bc, t3);
        const float dEdge = __builtin_fminf(__builtin_fminf(d1, d2), d3);
        const f3 nrm = cross(ab, ac);
        const float nn = dot(nrm, nrm), h = dot(ap, nrm);
        const float sw = dot(cross(ab, ap), nrm), sa = dot(cross(bc, bp), nrm), sv = dot(cross(ap, ac), nrm);
        const bool inside = nn > 0.f && sw >= 0.f && sa >= 0.f && sv >= 0.f;
        if (inside && (h * h) / nn < dEdge) { feature = 0.f; v = sv / nn; w = sw / nn; c = p - (h / nn) * nrm; }
        else if (d1 == dEdge) { feature = 1.f; v = t1; c = a + t1 * ab; }
        else if (d2 == dEdge) { feature = 2.f; w = t2; c = a + t2 * ac; }
        else { feature = 3.f; v = 1.f - t3; w = t3; c = (a + ab) + t3 * bc; }
        side = (h >= 0.f) ? 1.f : -1.f;
    }
    o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = v; o[4] = w; o[5] = side; o[6] = feature; o[7] = 0.f;
}

// A stack entry is int2 (bound, ref), bound = the bits of the child's boxdist2 (>= 0: they order as ints).
// Next entry whose bound is still within reach; false: the stack is empty
PT_DEV bool near_pop(const int2* stack, int& sp, float best, int& cur)
{
    while (sp > 0) {
        sp--;
        const int2 e = stack[sp * 64];
        if (!(__int_as_float(e.x) > best)) { cur = e.y; return true; }
    }
    return false;
}

// ---- the point walk of pt_knearest.hip's queries: candidates f(p, k) to a sink (pt_lists.h: SlotList has the interface) -----------
// Sinks: the K list, the count and the fill.  s.offer(f, prim): the sink's acceptance and, if it accepts, its take.  SINK::kOrdered:
// take the nearest child next (the bound falls sooner); else the children as they come.  SINK::kStops: the walk ends once s.done()
// (pt_lists.h: the any form's sink; false for every other sink, whose walks hold no such test).  pt_nearest.hip's closest query keeps its own
// copy of the walk (through this template its kernel's code changed and measured slower).

// The `cnt` triangles at tree position `first` (a leaf of either tree: ~ref = first << 3 | cnt)
template <class SINK>
PT_DEV void knear_leaf(const DevScene& sc, int ref, const f3& p, SINK& s)
{
    const int code = ~ref, first = code >> 3, cnt = code & 7;
    for (int k = 0; k < cnt; k++) {
        const float4* rec = sc.tri + 3 * (size_t)(first + k);
        const float4 a = rec[0], b = rec[1], c = rec[2];
        s.offer(tri_f(p, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z)), __float_as_int(a.w));
    }
}

// The walk over the 4-wide quantised tree.  A node pushes at most three of its children and descends into the fourth, a leaf pushes
// nothing: the stack never exceeds 3 entries per level (the caller has checked 3 * quad_depth + 2 <= kQueryStack), and the walk ends
// whatever the floats are, as quad_step's does.  An ordered sink takes the nearest child next and pushes the others farthest first.
template <class SINK>
PT_DEV void knear_walk_quad(const DevScene& sc, const f3& p, int2* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        if (cur >= 0) {
            const uint4* np = sc.quad + 4 * (size_t)cur;
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            const int ref[4] = {(int)n1.x, (int)n1.y, (int)n1.z, (int)n1.w};
            int key[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                f3 lo, hi;
                near_quad_child_box(n0, n2, n3, k, lo, hi);
                const float lb = boxdist2(p, lo, hi);
                key[k] = ((ref[k] == -1) | (lb > s.bound)) ? kQuadMiss : __float_as_int(lb);      // strictly: an equal bound may hide a tie that enters
            }
            if constexpr (SINK::kOrdered) {
                int k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3], r0 = ref[0], r1 = ref[1], r2 = ref[2], r3 = ref[3];
#define PT_CE(ka, ra, kb, rb) { const bool sw = ka > kb; const int tk = sw ? kb : ka, tr = sw ? rb : ra; kb = sw ? ka : kb; rb = sw ? ra : rb; ka = tk; ra = tr; }
                PT_CE(k0, r0, k1, r1) PT_CE(k2, r2, k3, r3) PT_CE(k0, r0, k2, r2) PT_CE(k1, r1, k3, r3) PT_CE(k1, r1, k2, r2)
#undef PT_CE
                if (k0 != kQuadMiss) {
                    if (k3 != kQuadMiss) { stack[sp * 64] = make_int2(k3, r3); sp++; }
                    if (k2 != kQuadMiss) { stack[sp * 64] = make_int2(k2, r2); sp++; }
                    if (k1 != kQuadMiss) { stack[sp * 64] = make_int2(k1, r1); sp++; }
                    cur = r0;
                    continue;
                }
            } else {
                bool have = false;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (key[k] == kQuadMiss) continue;
                    if (have) { stack[sp * 64] = make_int2(key[k], ref[k]); sp++; }
                    else { cur = ref[k]; have = true; }
                }
                if (have) continue;
            }
        } else {
            knear_leaf(sc, cur, p, s);
            if constexpr (SINK::kStops) { if (s.done()) return; }
        }
        if (!near_pop(stack, sp, s.bound, cur)) return;
    }
}

// The walk over the binary tree, for a scene whose 4-wide walk would not fit kQueryStack (or PTAMD_QUERY_QUAD=0).  As in trace_closest a
// leaf child is evaluated on the spot and an entry is pushed only where both children are interior: at most depth - 1 <= 31 entries.
template <class SINK>
PT_DEV void knear_walk_binary(const DevScene& sc, const f3& p, int2* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        if constexpr (SINK::kStops) { if (s.done()) return; }
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        f3 loL(q0.x, q0.y, q0.z), hiL(q0.w, q1.x, q1.y), loR(q1.z, q1.w, q2.x), hiR(q2.y, q2.z, q2.w);
        widen_binary(loL, hiL);
        widen_binary(loR, hiR);
        const float lbL = boxdist2(p, loL, hiL), lbR = boxdist2(p, loR, hiR);
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        if (refL < 0 && !(lbL > s.bound)) knear_leaf(sc, refL, p, s);
        if (refR < 0 && !(lbR > s.bound)) knear_leaf(sc, refR, p, s);
        const bool okL = (refL >= 0) & !(lbL > s.bound), okR = (refR >= 0) & !(lbR > s.bound);      // against what the leaves left
        if (okL & okR) {
            const bool lNear = !SINK::kOrdered || lbL <= lbR;
            stack[sp * 64] = lNear ? make_int2(__float_as_int(lbR), refR) : make_int2(__float_as_int(lbL), refL);
            sp++;
            cur = lNear ? refL : refR;
        } else if (okL) {
            cur = refL;
        } else if (okR) {
            cur = refR;
        } else if (!near_pop(stack, sp, s.bound, cur)) {
            return;
        }
    }
}

// Point q (p.xyz radius): the walk, then the spheres in order
template <bool QUAD, class SINK>
PT_DEV void knear_point(const DevScene& sc, const float4& q, int2* stack, SINK& s)
{
    const f3 p(q.x, q.y, q.z);
    if (QUAD) knear_walk_quad(sc, p, stack, s);
    else knear_walk_binary(sc, p, stack, s);
    for (int j = 0; j < sc.n_spheres; j++) s.offer(sphere_f(p, sc.spheres[4 * j]), sc.n_tris + j);
}

}  // namespace ptd

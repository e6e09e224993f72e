// pt_sweep.h — what the sphere casts are made of (pt_sweep.hip: pt_sweep_spheres; include/pt_api.h: "Sphere casts"; DESIGN.md section
// 43): the ONE statement of the float32 first-contact parameter tau(S, k) of a sweep S = (o, r, d, tmax) — the sphere of radius r whose
// centre moves along o + t d, t in [0, tmax] — and a primitive k, of the node test its walks prune with, and the ordered walks over
// either tree that hand the candidates to a query's sink.
//
// Why the cull is exact.  A member of a sweep is a primitive with tau <= bound, and tau is 0 only where f(o, k) <= r2 and otherwise at
// least tn of the record's own box inflated by r (step 2 of the header: a floor, as boxdist2 is f's).  The node test enters a box (lo,
// hi) iff boxdist2(o, lo, hi) <= r2, or the same slab test on [lo - r, hi + r] passes with its tn not above the bound.  Every operation of
// both tests — a subtraction, a product with the lane's fixed inv, a min, a max, a comparison — is monotone in lo and in hi under
// rounding to nearest, for fixed o, inv and r: a box that contains another has a boxdist2 not above, a tn not above and a tf not below
// the other's, in FLOAT32 and with no slack.  Every widened box of either tree contains the boxes of the records below it (section
// 29).  So a parent's interval contains a child's, and a culled node holds no member with tau <= bound: the argument of boxdist2
// (pt_nearest.hip) and of convex_overlaps (pt_convex.h).  The comparison with the bound is strict, tn > bound culls: an equal bound
// may hide a tie that the larger index wins.
//
// min and max are selects here, sw_min(a, b) = b < a ? b : a and sw_max(a, b) = b > a ? b : a: one answer for a NaN and for zeros of
// either sign on every compiler, which fminf does not promise.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_nearest.h"
#include "pt_box.h"

namespace ptd {

// ---- self-contained: begin (no helper of pt_math.h: tools/sweep_host.cpp compiles this text for the host, and tests/test_sweep.py holds
// it to the numpy restatement of tests/sweep_ref.py bit for bit) --------------------------------------------------------------------
// A contact that the rounding puts before the start (the sphere is not on the primitive by f, yet a candidate has begun) is taken NOW:
// at the smallest positive normal float, so that tau = 0 stays the statement of the point queries, f(o, k) <= r2, and of nothing else
#define PT_SWEEP_NOW 1.17549435e-38f
PT_DEV float sw_min(float a, float b) { return (b < a) ? b : a; }
PT_DEV float sw_max(float a, float b) { return (b > a) ? b : a; }
PT_DEV float sw_dot(const f3& a, const f3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PT_DEV f3 sw_sub(const f3& a, const f3& b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_DEV f3 sw_add(const f3& a, const f3& b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_DEV f3 sw_mad(const f3& a, float t, const f3& e) { return f3(a.x + t * e.x, a.y + t * e.y, a.z + t * e.z); }      // a + t e
PT_DEV f3 sw_msub(const f3& a, float t, const f3& e) { return f3(a.x - t * e.x, a.y - t * e.y, a.z - t * e.z); }     // a - t e
PT_DEV f3 sw_cross(const f3& a, const f3& b) { return f3(a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x); }

// boxdist2 of the closest-point section
PT_DEV float sw_boxdist2(const f3& p, const f3& lo, const f3& hi)
{
    const float gx = sw_max(sw_max(lo.x - p.x, p.x - hi.x), 0.f);
    const float gy = sw_max(sw_max(lo.y - p.y, p.y - hi.y), 0.f);
    const float gz = sw_max(sw_max(lo.z - p.z, p.z - hi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// seg of the closest-point section, the distance alone
PT_DEV float sw_seg(const f3& q, const f3& e)
{
    float t = sw_dot(q, e) / sw_dot(e, e);
    t = (t > 0.f) ? t : 0.f;
    t = (t < 1.f) ? t : 1.f;
    const f3 r = sw_msub(q, t, e);
    return sw_dot(r, r);
}

// Are the three edge functions of f's `inside` all >= 0 at the point a + ap?  (nn > 0 is the caller's)
PT_DEV bool sw_inside(const f3& ap, const f3& ab, const f3& ac, const f3& bc, const f3& n)
{
    const f3 bp = sw_sub(ap, ab);
    return sw_dot(sw_cross(ab, ap), n) >= 0.f && sw_dot(sw_cross(bc, bp), n) >= 0.f && sw_dot(sw_cross(ap, ac), n) >= 0.f;
}

// first(m, dv, R2) of the header: the first touch of the line m + t dv with the ball of squared radius R2 about 0, by the closest
// approach t0; a line that has entered the ball already and still approaches its middle touches NOW; +inf: no touch at t >= 0
PT_DEV float sw_first(const f3& m, const f3& dv, float R2)
{
    const float A = sw_dot(dv, dv);
    const float t0 = -sw_dot(m, dv) / A;
    const f3 w = sw_mad(m, t0, dv);
    const float k = R2 - sw_dot(w, w);
    const float t = t0 - __builtin_sqrtf(k / A);
    return (A > 0.f && k >= 0.f && t0 >= 0.f) ? sw_max(PT_SWEEP_NOW, t) : __builtin_inff();
}

// Step 2 of the header on the box (lo, hi) inflated by r: does every axis pass with tn <= tf?  tn: the entry parameter, >= +0.
// inv = 1 / d per axis (read only where d != 0).
PT_DEV bool sweep_slab(const f3& o, const f3& d, const f3& inv, float r, float tmax, const f3& lo, const f3& hi, float& tn)
{
    bool pass = true;
    float n = 0.f, f = tmax;
    {
        const float l = lo.x - r, h = hi.x + r;
        if (d.x != 0.f) {
            const float t1 = (l - o.x) * inv.x, t2 = (h - o.x) * inv.x;
            n = sw_max(n, sw_min(t1, t2));
            f = sw_min(f, sw_max(t1, t2));
        } else {
            pass &= (l <= o.x) & (o.x <= h);
        }
    }
    {
        const float l = lo.y - r, h = hi.y + r;
        if (d.y != 0.f) {
            const float t1 = (l - o.y) * inv.y, t2 = (h - o.y) * inv.y;
            n = sw_max(n, sw_min(t1, t2));
            f = sw_min(f, sw_max(t1, t2));
        } else {
            pass &= (l <= o.y) & (o.y <= h);
        }
    }
    {
        const float l = lo.z - r, h = hi.z + r;
        if (d.z != 0.f) {
            const float t1 = (l - o.z) * inv.z, t2 = (h - o.z) * inv.z;
            n = sw_max(n, sw_min(t1, t2));
            f = sw_min(f, sw_max(t1, t2));
        } else {
            pass &= (l <= o.z) & (o.z <= h);
        }
    }
    tn = n;
    return pass & (n <= f);
}

// The node test: may anything below the box (lo, hi) be a member with tau <= bound?  key: what the ordered walk sorts the box by, 0
// where the sphere at its start may reach into the box, else tn.
PT_DEV bool sweep_node_test(const f3& o, const f3& d, const f3& inv, float r, float r2, float tmax, float bound, const f3& lo, const f3& hi, float& key)
{
    key = 0.f;
    if (sw_boxdist2(o, lo, hi) <= r2) return true;
    float tn;
    if (!sweep_slab(o, d, inv, r, tmax, lo, hi, tn)) return false;
    key = tn;
    return !(tn > bound);
}

// tau(S, triangle) of the header, operation for operation; +inf: no contact within tmax.  bound: a result above it is of no use to the
// caller, so a record whose own tn exceeds it returns +inf before its candidates (tau >= tn: nothing the sink would take is lost);
// bound = tmax gives tau itself.
PT_DEV float sweep_tri_key(const f3& o, const f3& d, const f3& inv, float r, float r2, float tmax, float bound, const f3& a, const f3& ab, const f3& ac)
{
    const float kInf = __builtin_inff();
    const f3 b = sw_add(a, ab), c = sw_add(a, ac), bc = sw_sub(ac, ab);
    const f3 tlo(sw_min(sw_min(a.x, b.x), c.x), sw_min(sw_min(a.y, b.y), c.y), sw_min(sw_min(a.z, b.z), c.z));
    const f3 thi(sw_max(sw_max(a.x, b.x), c.x), sw_max(sw_max(a.y, b.y), c.y), sw_max(sw_max(a.z, b.z), c.z));
    const f3 n = sw_cross(ab, ac), oa = sw_sub(o, a);
    const float nn = sw_dot(n, n), h = sw_dot(oa, n);
    // 1. overlap at the start: f(o, k) <= r2.  f >= boxdist2 of the record's box exactly, so beyond it f need not be formed.
    const float floor2 = sw_boxdist2(o, tlo, thi);
    if (floor2 <= r2) {
        const float dEdge = sw_min(sw_min(sw_seg(oa, ab), sw_seg(oa, ac)), sw_seg(sw_sub(oa, ab), bc));
        const bool inside = nn > 0.f && sw_inside(oa, ab, ac, bc, n);
        const float dPlane = (h * h) / nn;
        const float dRaw = (inside && dPlane < dEdge) ? dPlane : dEdge;
        if (sw_max(dRaw, floor2) <= r2) return 0.f;
    }
    if (bound < PT_SWEEP_NOW) return kInf;      // every contact below is at NOW or later: a sink that holds a tau = 0 wants none of them
    // 2. the floor: the record's own box inflated by r
    float tn;
    if (!sweep_slab(o, d, inv, r, tmax, tlo, thi, tn)) return kInf;
    if (tn > bound) return kInf;
    // 3. the candidates: the near face offset by r, the three edge cylinders, the three vertex balls
    float best = kInf;
    {
        const float dn = sw_dot(d, n);
        const float s = (h >= 0.f) ? 1.f : -1.f;
        const float ln = __builtin_sqrtf(nn);
        const float g = s * h - r * ln, sdn = s * dn;
        if (nn > 0.f && sdn < 0.f) {
            const float t = sw_max(PT_SWEEP_NOW, (g > 0.f) ? g / -sdn : 0.f);      // within r of the plane already: contact now, if q is on the face
            const f3 q = sw_msub(sw_mad(o, t, d), (s * r) / ln, n);
            if (sw_inside(sw_sub(q, a), ab, ac, bc, n)) best = sw_min(best, t);
        }
    }
    {
        const float ee = sw_dot(ab, ab);
        if (ee > 0.f) {
            const float um = sw_dot(oa, ab) / ee, ud = sw_dot(d, ab) / ee;
            const float t = sw_first(sw_msub(oa, um, ab), sw_msub(d, ud, ab), r2);
            const float u = um + t * ud;
            if (0.f <= u && u <= 1.f) best = sw_min(best, t);
        }
    }
    {
        const float ee = sw_dot(ac, ac);
        if (ee > 0.f) {
            const float um = sw_dot(oa, ac) / ee, ud = sw_dot(d, ac) / ee;
            const float t = sw_first(sw_msub(oa, um, ac), sw_msub(d, ud, ac), r2);
            const float u = um + t * ud;
            if (0.f <= u && u <= 1.f) best = sw_min(best, t);
        }
    }
    const f3 ob = sw_sub(o, b);
    {
        const float ee = sw_dot(bc, bc);
        if (ee > 0.f) {
            const float um = sw_dot(ob, bc) / ee, ud = sw_dot(d, bc) / ee;
            const float t = sw_first(sw_msub(ob, um, bc), sw_msub(d, ud, bc), r2);
            const float u = um + t * ud;
            if (0.f <= u && u <= 1.f) best = sw_min(best, t);
        }
    }
    best = sw_min(best, sw_first(oa, d, r2));
    best = sw_min(best, sw_first(ob, d, r2));
    best = sw_min(best, sw_first(sw_sub(o, c), d, r2));
    // 4. never before the floor
    const float tau = sw_max(best, tn);
    return (tau <= tmax) ? tau : kInf;
}

// tau(S, sphere) of the header: ctr.xyz | rad; contact is with the sphere's surface, from outside or from within
PT_DEV float sweep_sphere_key(const f3& o, const f3& d, float r, float r2, float tmax, const f3& ctr, float rad)
{
    const float kInf = __builtin_inff();
    const f3 pc = sw_sub(o, ctr);
    const float l = __builtin_sqrtf(sw_dot(pc, pc));
    const float g = l - rad;
    if (g * g <= r2) return 0.f;
    float tau;
    if (l > rad) {
        const float R = rad + r;
        tau = sw_first(pc, d, R * R);
    } else {      // deep inside the ball: the centre leaves the ball of radius rad - r
        const float R = rad - r;
        const float A = sw_dot(d, d);
        const float t0 = -sw_dot(pc, d) / A;
        const f3 w = sw_mad(pc, t0, d);
        const float k = R * R - sw_dot(w, w);
        const float t = t0 + __builtin_sqrtf(k / A);
        tau = (A > 0.f && k >= 0.f) ? sw_max(PT_SWEEP_NOW, t) : kInf;
    }
    return (tau <= tmax) ? tau : kInf;
}
// ---- self-contained: end ------------------------------------------------------------------------------------------------------------

// A lane's sweep, in registers: the SWEEP8 record, inv = 1 / d per axis and r2 = r * r
struct SweepLane {
    f3 o, d, inv;
    float r, r2, tmax;
};

PT_DEV SweepLane sweep_lane(const float4& q0, const float4& q1)
{
    SweepLane q;
    q.o = f3(q0.x, q0.y, q0.z);
    q.d = f3(q1.x, q1.y, q1.z);
    q.inv = f3(1.f / q1.x, 1.f / q1.y, 1.f / q1.z);
    q.r = q0.w;
    q.r2 = q0.w * q0.w;
    q.tmax = q1.w;
    return q;
}

// A candidate to a sink (pt_lists.h): wants(), then take().  tau = +inf is no member, whatever tmax is.
template <class SINK>
PT_DEV void sweep_offer(SINK& s, float tau, int prim)
{
    if (tau < __builtin_inff() && s.wants(tau, prim)) s.take(tau, prim);
}

// The node test as a stack key: the bits of `key` (>= +0: they order as ints), kQuadMiss for a box the sweep passes by whatever the
// bound; sweep_reach: the rest of the test, against the bound as it is now
PT_DEV int sweep_node_key(const SweepLane& q, const f3& lo, const f3& hi)
{
    float key;
    return sweep_node_test(q.o, q.d, q.inv, q.r, q.r2, q.tmax, __builtin_inff(), lo, hi, key) ? __float_as_int(key) : kQuadMiss;
}
PT_DEV bool sweep_reach(int key, float bound) { return (key != kQuadMiss) & !(__int_as_float(key) > bound); }

// The `cnt` triangles at tree position `first` (a leaf of either tree: ~ref = first << 3 | cnt)
template <class SINK>
PT_DEV void sweep_leaf(const DevScene& sc, int ref, const SweepLane& q, SINK& s)
{
    const int code = ~ref, first = code >> 3, cnt = code & 7;
    for (int k = 0; k < cnt; k++) {
        const float4* rec = sc.tri + 3 * (size_t)(first + k);
        const float4 a = rec[0], b = rec[1], c = rec[2];
        sweep_offer(s, sweep_tri_key(q.o, q.d, q.inv, q.r, q.r2, q.tmax, s.bound, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z)), __float_as_int(a.w));
    }
}

// The ordered walk over the 4-wide quantised tree, knear_walk_quad's with the sweep's node test: the nearest child next, the others
// pushed farthest first as int2 (key bits, ref) at stack[e * 64]; at most 3 entries per level (the caller has checked 3 * quad_depth + 2
// <= kQueryStack); a popped entry whose key exceeds the bound by now is dropped without fetching its node.
template <class SINK>
PT_DEV void sweep_walk_quad(const DevScene& sc, const SweepLane& q, int2* stack, SINK& s)
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
                const int kk = sweep_node_key(q, lo, hi);
                key[k] = ((ref[k] != -1) & sweep_reach(kk, s.bound)) ? kk : kQuadMiss;      // an empty slot's box is inverted, not far away
            }
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
            sweep_leaf(sc, cur, q, s);
            if constexpr (SINK::kStops) { if (s.done()) return; }
        }
        if (!near_pop(stack, sp, s.bound, cur)) return;
    }
}

// The ordered walk over the binary tree, knear_walk_binary's with the sweep's node test: a leaf child is evaluated on the spot, an
// entry is pushed only where both children are interior: at most depth - 1 <= 31 entries
template <class SINK>
PT_DEV void sweep_walk_binary(const DevScene& sc, const SweepLane& q, int2* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        if constexpr (SINK::kStops) { if (s.done()) return; }
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        f3 loL(q0.x, q0.y, q0.z), hiL(q0.w, q1.x, q1.y), loR(q1.z, q1.w, q2.x), hiR(q2.y, q2.z, q2.w);
        widen_binary(loL, hiL);
        widen_binary(loR, hiR);
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        const int kL = sweep_node_key(q, loL, hiL), kR = sweep_node_key(q, loR, hiR);
        if (refL < 0 && sweep_reach(kL, s.bound)) sweep_leaf(sc, refL, q, s);
        if (refR < 0 && sweep_reach(kR, s.bound)) sweep_leaf(sc, refR, q, s);
        const bool okL = (refL >= 0) & sweep_reach(kL, s.bound), okR = (refR >= 0) & sweep_reach(kR, s.bound);      // against what the leaves left
        if (okL & okR) {
            const bool lNear = kL <= kR;
            stack[sp * 64] = lNear ? make_int2(kR, refR) : make_int2(kL, refL);
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

// Sweep q: the walk, then the spheres in order
template <bool QUAD, class SINK>
PT_DEV void sweep_query(const DevScene& sc, const SweepLane& q, int2* stack, SINK& s)
{
    if (QUAD) sweep_walk_quad(sc, q, stack, s);
    else sweep_walk_binary(sc, q, stack, s);
    for (int j = 0; j < sc.n_spheres; j++) {
        if constexpr (SINK::kStops) { if (s.done()) return; }
        const float4 sp = sc.spheres[4 * j];
        sweep_offer(s, sweep_sphere_key(q.o, q.d, q.r, q.r2, q.tmax, f3(sp.x, sp.y, sp.z), sp.w), sc.n_tris + j);
    }
}

}  // namespace ptd

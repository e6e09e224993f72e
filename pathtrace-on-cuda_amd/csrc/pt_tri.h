// pt_tri.h — what the triangle queries are made of (pt_tri.hip: pt_tri_count, pt_tri_any, pt_tri_list; include/pt_api.h: "Triangle
// queries"): the ONE statement of the float32 membership of a query triangle T = (qa, qb, qc) and a primitive k
// with its section segment p .. q, of the node test the walks cull with, and the unordered bare-ref walks over either tree that hand
// every primitive below an entered leaf to a query's sink.
//
// Why the cull is exact.  A triangle k is a member only if (1) its record's own box overlaps T's own box on every axis and (2) one of
// its vertices has d(v) >= 0 and one has not, d being T's plane function.  The node test enters a box (lo, hi) iff it overlaps T's box
// by the same comparisons and straddles the plane: d at the corner that minimises it (per axis lo where n >= 0, hi otherwise) is < 0
// and d at the opposite corner is >= 0.
//   - d(v) = (n.x*(v.x - qa.x) + n.y*(v.y - qa.y)) + n.z*(v.z - qa.z): a subtraction of the lane's fixed qa, a product with the lane's
//     fixed n, two sums.  Each is monotone in every coordinate of v under rounding to nearest (non-decreasing where that component of
//     n is >= 0, non-increasing otherwise), so in FLOAT32 and with no slack d(min corner) <= d(v) <= d(max corner) for every float
//     point v of the box.
//   - The three vertices a, a + E1, a + E2 of a record, as the key forms them, lie in the record's own box (it is their min and max),
//     and every widened box of either tree contains the boxes of the records below it (section 29).
//   - So below a box with d(min corner) >= 0 every vertex is above, below one with d(max corner) < 0 none is, and below one that
//     misses T's box every record box does: a culled node holds no member.  This is convex_overlaps' argument (pt_convex.h) applied
//     to one plane from both sides, and box_overlaps' (pt_box.h).  A NaN in the query makes every d NaN: no comparison passes, in the
//     key or in the node test.
// Nothing is ordered (a node test has no distance), a stack entry is a bare ref, and no popped entry is tested again.
//
// min and max are selects, as in pt_sweep.h: one answer for a NaN and for zeros of either sign on every compiler.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_nearest.h"
#include "pt_box.h"

namespace ptd {

// ---- self-contained: begin (no helper of pt_math.h: tools/tri_host.cpp compiles this text for the host, and tests/test_tri_queries.py
// holds it to the numpy restatement of tests/tri_ref.py bit for bit) -----------------------------------------------------------------
PT_DEV float tq_min(float a, float b) { return (b < a) ? b : a; }
PT_DEV float tq_max(float a, float b) { return (b > a) ? b : a; }
PT_DEV float tq_dot(const f3& a, const f3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PT_DEV f3 tq_sub(const f3& a, const f3& b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_DEV f3 tq_add(const f3& a, const f3& b) { return f3(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_DEV f3 tq_mad(const f3& a, float t, const f3& e) { return f3(a.x + t * e.x, a.y + t * e.y, a.z + t * e.z); }      // a + t e
PT_DEV f3 tq_cross(const f3& a, const f3& b) { return f3(a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x); }
PT_DEV f3 tq_min3(const f3& a, const f3& b, const f3& c)
{
    return f3(tq_min(tq_min(a.x, b.x), c.x), tq_min(tq_min(a.y, b.y), c.y), tq_min(tq_min(a.z, b.z), c.z));
}
PT_DEV f3 tq_max3(const f3& a, const f3& b, const f3& c)
{
    return f3(tq_max(tq_max(a.x, b.x), c.x), tq_max(tq_max(a.y, b.y), c.y), tq_max(tq_max(a.z, b.z), c.z));
}

// What a lane keeps of its query T = (qa, qb, qc): qa, the plane normal n = cross(qb - qa, qc - qa), T's own box, the inward normals
// m_i = cross(n, e_i) of the edges e_0 = qb - qa, e_1 = qc - qb, e_2 = qa - qc — and qb, the point edge 1 is measured from (edges 0
// and 2 pass through qa): 24 floats
struct TriLane {
    f3 qa, qb, n, lo, hi, m0, m1, m2;
};

PT_DEV TriLane tri_lane(const f3& qa, const f3& qb, const f3& qc)
{
    TriLane L;
    L.qa = qa;
    L.qb = qb;
    L.n = tq_cross(tq_sub(qb, qa), tq_sub(qc, qa));
    L.lo = tq_min3(qa, qb, qc);
    L.hi = tq_max3(qa, qb, qc);
    L.m0 = tq_cross(L.n, tq_sub(qb, qa));
    L.m1 = tq_cross(L.n, tq_sub(qc, qb));
    L.m2 = tq_cross(L.n, tq_sub(qa, qc));
    return L;
}

// d(v) of the header: T's plane function, in the order written
PT_DEV float tri_plane(const TriLane& L, const f3& v)
{
    return (L.n.x * (v.x - L.qa.x) + L.n.y * (v.y - L.qa.y)) + L.n.z * (v.z - L.qa.z);
}

// One clip of the header's step 4: the segment P .. Q, parameter interval [s0, s1], against the edge function w(x) = dot(m, x - v),
// inside where w >= 0.  false: both ends are outside — no member.
PT_DEV bool tri_clip(const f3& m, const f3& v, const f3& P, const f3& Q, float& s0, float& s1)
{
    const float wp = tq_dot(m, tq_sub(P, v)), wq = tq_dot(m, tq_sub(Q, v));
    const bool ip = wp >= 0.f, iq = wq >= 0.f;
    if (!ip && !iq) return false;
    if (ip != iq) {
        const float s = wp / (wp - wq);
        if (ip) s1 = tq_min(s1, s);
        else s0 = tq_max(s0, s);
    }
    return true;
}

// The key of T and the triangle record (a, ab, ac): 1 = member, with its section segment p .. q; +inf = no member (p, q untouched)
PT_DEV float tri_tri_key(const TriLane& L, const f3& a, const f3& ab, const f3& ac, f3& p, f3& q)
{
    const float kNone = __builtin_inff();
    const f3 b = tq_add(a, ab), c = tq_add(a, ac);
    // 1. the box floor
    const f3 tlo = tq_min3(a, b, c), thi = tq_max3(a, b, c);
    if (!(tlo.x <= L.hi.x && thi.x >= L.lo.x && tlo.y <= L.hi.y && thi.y >= L.lo.y && tlo.z <= L.hi.z && thi.z >= L.lo.z)) return kNone;
    // 2. the plane floor: one vertex above (d >= 0), one not
    const float da = tri_plane(L, a), db = tri_plane(L, b), dc = tri_plane(L, c);
    const bool ua = da >= 0.f, ub = db >= 0.f, uc = dc >= 0.f;
    if (ua == ub && ub == uc) return kNone;
    // 3. the section: the lone vertex l and the other two in cyclic order
    f3 l, v1, v2;
    float dl, d1, d2;
    if (ua != ub && ua != uc) { l = a; v1 = b; v2 = c; dl = da; d1 = db; d2 = dc; }
    else if (ub != ua && ub != uc) { l = b; v1 = c; v2 = a; dl = db; d1 = dc; d2 = da; }
    else { l = c; v1 = a; v2 = b; dl = dc; d1 = da; d2 = db; }
    const float t1 = dl / (dl - d1), t2 = dl / (dl - d2);
    const f3 P = tq_mad(l, t1, tq_sub(v1, l)), Q = tq_mad(l, t2, tq_sub(v2, l));
    // 4. the clip against T's three edges
    float s0 = 0.f, s1 = 1.f;
    if (!tri_clip(L.m0, L.qa, P, Q, s0, s1)) return kNone;
    if (!tri_clip(L.m1, L.qb, P, Q, s0, s1)) return kNone;
    if (!tri_clip(L.m2, L.qa, P, Q, s0, s1)) return kNone;
    if (!(s0 <= s1)) return kNone;
    const f3 PQ = tq_sub(Q, P);
    p = tq_mad(P, s0, PQ);
    q = tq_mad(P, s1, PQ);
    return 1.f;
}

// seg of the closest-point section with its parameter
PT_DEV float tq_seg(const f3& q, const f3& e, float& t)
{
    t = tq_dot(q, e) / tq_dot(e, e);
    t = (t > 0.f) ? t : 0.f;
    t = (t < 1.f) ? t : 1.f;
    const f3 r = f3(q.x - t * e.x, q.y - t * e.y, q.z - t * e.z);
    return tq_dot(r, r);
}

// f(p, triangle) of the closest-point section for the triangle (a, ab, ac) with its closest point c as the detail record forms it
// (min and max as selects)
PT_DEV float tq_closest(const f3& p, const f3& a, const f3& ab, const f3& ac, f3& c)
{
    const f3 bc = tq_sub(ac, ab), ap = tq_sub(p, a), bp = tq_sub(ap, ab);
    float t1, t2, t3;
    const float d1 = tq_seg(ap, ab, t1), d2 = tq_seg(ap, ac, t2), d3 = tq_seg(bp, bc, t3);
    const float dEdge = tq_min(tq_min(d1, d2), d3);
    const f3 n = tq_cross(ab, ac);
    const float nn = tq_dot(n, n), h = tq_dot(ap, n);
    const float sw = tq_dot(tq_cross(ab, ap), n), sa = tq_dot(tq_cross(bc, bp), n), sv = tq_dot(tq_cross(ap, ac), n);
    const bool inside = nn > 0.f && sw >= 0.f && sa >= 0.f && sv >= 0.f;
    const float dPlane = (h * h) / nn;
    float dRaw = dEdge;
    if (inside && dPlane < dEdge) {
        const float u = h / nn;
        dRaw = dPlane;
        c = f3(p.x - u * n.x, p.y - u * n.y, p.z - u * n.z);
    } else if (d1 == dEdge) {
        c = tq_mad(a, t1, ab);
    } else if (d2 == dEdge) {
        c = tq_mad(a, t2, ac);
    } else {
        c = tq_mad(tq_add(a, ab), t3, bc);
    }
    const f3 b = tq_add(a, ab), cc = tq_add(a, ac);
    const f3 lo = tq_min3(a, b, cc), hi = tq_max3(a, b, cc);
    const float gx = tq_max(tq_max(lo.x - p.x, p.x - hi.x), 0.f), gy = tq_max(tq_max(lo.y - p.y, p.y - hi.y), 0.f),
                gz = tq_max(tq_max(lo.z - p.z, p.z - hi.z), 0.f);
    return tq_max(dRaw, (gx * gx + gy * gy) + gz * gz);
}

// The key of T = (qa, qb, qc) and the sphere (ctr, rad), membership by the SURFACE: T comes within rad of the centre and reaches out of
// the ball.  c: the point of T closest to the centre.
PT_DEV float tri_sphere_key(const f3& qa, const f3& qb, const f3& qc, const f3& ctr, float rad, f3& c)
{
    const float f = tq_closest(ctr, qa, tq_sub(qb, qa), tq_sub(qc, qa), c);
    const f3 va = tq_sub(qa, ctr), vb = tq_sub(qb, ctr), vc = tq_sub(qc, ctr);
    const float far2 = tq_max(tq_max(tq_dot(va, va), tq_dot(vb, vb)), tq_dot(vc, vc));
    const float rr = rad * rad;
    return (f <= rr && far2 >= rr) ? 1.f : __builtin_inff();
}

// May anything below the box (lo, hi) be a member of the lane's query?  (the proof is at the top of this file)
PT_DEV bool tri_node_test(const TriLane& L, const f3& lo, const f3& hi)
{
    if (!(lo.x <= L.hi.x && hi.x >= L.lo.x && lo.y <= L.hi.y && hi.y >= L.lo.y && lo.z <= L.hi.z && hi.z >= L.lo.z)) return false;
    const bool px = L.n.x >= 0.f, py = L.n.y >= 0.f, pz = L.n.z >= 0.f;
    const f3 cmin(px ? lo.x : hi.x, py ? lo.y : hi.y, pz ? lo.z : hi.z), cmax(px ? hi.x : lo.x, py ? hi.y : lo.y, pz ? hi.z : lo.z);
    return tri_plane(L, cmin) < 0.f && tri_plane(L, cmax) >= 0.f;
}
// ---- self-contained: end -------------------------------------------------------------------------------------------------------------

// The `cnt` triangles at tree position `first` (a leaf of either tree: ~ref = first << 3 | cnt), as box_leaf
template <class SINK>
PT_DEV void tri_leaf(const DevScene& sc, int ref, const TriLane& L, SINK& s)
{
    const int code = ~ref, first = code >> 3, cnt = code & 7;
    for (int k = 0; k < cnt; k++) {
        const float4* rec = sc.tri + 3 * (size_t)(first + k);
        const float4 a = rec[0], b = rec[1], c = rec[2];
        f3 p, q;
        box_offer(s, tri_tri_key(L, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z), p, q), __float_as_int(a.w));
    }
}

// The walk over the 4-wide quantised tree, box_walk_quad's shape with this file's node test: at most 3 entries per level (the caller
// has checked 3 * quad_depth + 2 <= kQueryStack), and it ends whatever the floats are.  Entry e of a lane's stack is stack[e * 64].
template <class SINK>
PT_DEV void tri_walk_quad(const DevScene& sc, const TriLane& L, int* stack, SINK& s)
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
                if ((ref[k] == -1) | !tri_node_test(L, clo, chi)) continue;
                if (have) { stack[sp * 64] = ref[k]; sp++; }
                else { cur = ref[k]; have = true; }
            }
            if (have) continue;
        } else {
            tri_leaf(sc, cur, L, s);
            if constexpr (SINK::kStops) { if (s.done()) return; }
        }
        if (sp == 0) return;
        sp--;
        cur = stack[sp * 64];
    }
}

// The walk over the binary tree, box_walk_binary's shape: a leaf child is evaluated on the spot and an entry is pushed only where both
// children are interior and pass: at most depth - 1 <= 31 entries.
template <class SINK>
PT_DEV void tri_walk_binary(const DevScene& sc, const TriLane& L, int* stack, SINK& s)
{
    int cur = 0, sp = 0;
    for (;;) {
        if constexpr (SINK::kStops) { if (s.done()) return; }
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        f3 loL(q0.x, q0.y, q0.z), hiL(q0.w, q1.x, q1.y), loR(q1.z, q1.w, q2.x), hiR(q2.y, q2.z, q2.w);
        widen_binary(loL, hiL);
        widen_binary(loR, hiR);
        const bool inL = tri_node_test(L, loL, hiL), inR = tri_node_test(L, loR, hiR);
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        if (refL < 0 && inL) tri_leaf(sc, refL, L, s);
        if (refR < 0 && inR) tri_leaf(sc, refR, L, s);
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

// Query T: the walk, then the spheres in order.  qc: T's third vertex, which the lane does not keep (the spheres' key takes T itself).
template <bool QUAD, class SINK>
PT_DEV void tri_query(const DevScene& sc, const TriLane& L, const f3& qc, int* stack, SINK& s)
{
    if (QUAD) tri_walk_quad(sc, L, stack, s);
    else tri_walk_binary(sc, L, stack, s);
    for (int j = 0; j < sc.n_spheres; j++) {
        const float4 sp = sc.spheres[4 * j];
        f3 c;
        box_offer(s, tri_sphere_key(L.qa, L.qb, qc, f3(sp.x, sp.y, sp.z), sp.w, c), sc.n_tris + j);
    }
}

// The 8-float detail record of the header for query T and member `prim`: p.xyz | q.xyz | kind | 0, recomputed from the scene's current
// records by the same functions — the same bits.  A triangle is read from its surface record (indexed by primitive, V0 E1 E2 first:
// the floats its tri record holds), as near_detail reads it.  A slot whose primitive is no member of T (a caller's own records) gets zeros.
PT_DEV void tri_detail(const DevScene& sc, const TriLane& L, const f3& qc, int prim, float* o)
{
    f3 p(0.f, 0.f, 0.f), q(0.f, 0.f, 0.f);
    float key, kind;
    if (prim >= sc.n_tris + sc.n_spheres) {      // no record of a fill: nothing is read
        key = 0.f;
        kind = 0.f;
    } else if (prim >= sc.n_tris) {
        const float4 sp = sc.spheres[4 * (prim - sc.n_tris)];
        key = tri_sphere_key(L.qa, L.qb, qc, f3(sp.x, sp.y, sp.z), sp.w, p);
        q = p;
        kind = 2.f;
    } else {
        const float4* rec = sc.surf + 12 * (size_t)prim;
        const float4 s0 = rec[0], s1 = rec[1], s2 = rec[2];
        key = tri_tri_key(L, f3(s0.x, s0.y, s0.z), f3(s0.w, s1.x, s1.y), f3(s1.z, s1.w, s2.x), p, q);
        kind = 1.f;
    }
    const bool member = key == 1.f;
    o[0] = member ? p.x : 0.f; o[1] = member ? p.y : 0.f; o[2] = member ? p.z : 0.f;
    o[3] = member ? q.x : 0.f; o[4] = member ? q.y : 0.f; o[5] = member ? q.z : 0.f;
    o[6] = member ? kind : 0.f; o[7] = 0.f;
}

}  // namespace ptd

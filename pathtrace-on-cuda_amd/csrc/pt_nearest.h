// pt_nearest.h — what the distance queries share (pt_nearest.hip: pt_closest_points; pt_knearest.hip: pt_nearest_k, pt_count_within): the
// ONE statement of the float32 function f of include/pt_api.h ("Closest-point queries"), of the box distance their walks prune with,
// of the widening of the child boxes of either tree that the pruning's premise rests on, and of the detail record.
// DESIGN.md sections 29 and 30.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"

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

}  // namespace ptd

// pt_rayhits.hip — the first K hits along each of the caller's rays, sorted, and the number of hits, on an uploaded scene
// (include/pt_api.h: pt_trace_rays_k, pt_count_hits).  DESIGN.md section 34.
//
// Both are DEFINED without a tree, over H(ray) = the (t, prim, facing) records the header's acceptance rules admit in [0, tmax]: the
// first K members of H in the order (t ascending as floats, among equal t the larger prim first), and |H|.  The walks only have to
// find them.  A box on the way to a member at t is entered by the ray no later than t (in the walk's units, with the slack the
// closest-hit walk already relies on), so a child culled at `bound` holds no member at t <= bound: quad_step's argument with the
// closest hit replaced by the sink's bound — tmax while the list holds fewer than K, then the t of its last slot (it only ever
// decreases); for the count it is tmax throughout.  The cull lets a box through whose entry EQUALS the bound, so a tie at the bound
// is still met and the tie rule decides.  As in pt_knearest.hip every triangle must sit below exactly ONE leaf of the tree walked.
//
// Shape: query_rays' (pt_query.hip) — one ray per lane, one-wave workgroups, the per-lane int stack in LDS with entry e at
// stack[e * 64].  Beside it nearest_k's per-lane list, sorted, slot j at list[j * kSlotRow + lane] as int2 (t's bits, prim): pt_lists.h's
// SlotList<true>, t compared as a FLOAT (-0 equals +0, and its bits go out as pt_trace_rays would write them).  Facing is not stored: the detail kernel
// recomputes it from the sign of det (a triangle) or from which root the slot holds (a sphere).
#include <hip/hip_runtime.h>
#include "pt_device.h"
#include "pt_math.h"
#include "pt_trace.h"
#include "pt_scene.h"
#include "pt_lists.h"

namespace ptd {

// What a walk hands its hits to (pt_lists.h: SlotList has the interface; wants() is asked before the leaf box is fetched).
// |H|: the bound stays tmax.  counts(): its acceptance, and the fill's for a long segment (pt_lists.h: SlotSeg).
struct HitCount {
    static constexpr bool kStops = false;
    int cnt;
    float bound;
    PT_DEV static bool counts(float t, float bound) { return !(t > bound); }
    PT_DEV bool wants(float t, int) const { return counts(t, bound); }
    PT_DEV void take(float, int) { cnt++; }
};

// One triangle of a binary-tree leaf, from its tri record: tri_test's arithmetic and test order (pt_trace.h), the two-sided rule of
// tri_hits_pairrec, the sink's precondition before the reference leaf box.
template <bool BOTH, class SINK>
PT_DEV void tri_hits(const DevScene& sc, int q, const f3& org, const f3& dir, const f3& invD, bool degenerate, SINK& s)
{
    const float4 a = sc.tri[3 * (size_t)q], b = sc.tri[3 * (size_t)q + 1], c = sc.tri[3 * (size_t)q + 2];
    const f3 V0(a.x, a.y, a.z), E1(b.x, b.y, b.z), E2(c.x, c.y, c.z);
    const f3 T = org - V0;
    const f3 P = cross(dir, E2);
    const f3 Q = cross(T, E1);
    float det = dot(P, E1);
    const bool back = BOTH & (det < kEps);
    const float t = dot(Q, E2) * (1.f / det);
    float u = dot(P, T), v = dot(Q, dir);
    if (back) { det = -det; u = -u; v = -v; }
    if (det < kEps) return;
    if (t < 0.f) return;
    if (u < 0.f || u > det) return;
    if (v < 0.f || (v + u) > det) return;
    const int prim = __float_as_int(a.w);
    if (!s.wants(t, prim)) return;
    if (!degenerate) {
        const int leaf = __float_as_int(b.w);
        const float4 l0 = sc.leafbox[2 * leaf], l1 = sc.leafbox[2 * leaf + 1];
        float tn;
        if (!box_test(l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, org, invD, __builtin_inff(), tn)) return;
    }
    s.take(t, prim);
}

// The walk over the 4-wide quantised tree: quad_step's (pt_trace.h) with the sink's bound where the closest hit was, and no early
// out.  A node pushes at most three of its children and descends into the fourth, a leaf pushes nothing: at most 3 entries per
// level (the caller has checked 3 * quad_depth + 2 <= kQueryStack), and the walk ends whatever the floats are.
template <bool BOTH, class SINK>
PT_DEV void hits_walk_quad(const DevScene& sc, const f3& org, const f3& dir, int* stack, SINK& s)
{
    f3 inv; float cscale; bool degenerate;
    ray_setup(dir, inv, cscale, degenerate);
    int cur = 0, sp = 0;
    for (;;) {
        if (cur >= 0) {
            const uint4* np = sc.quad + 4 * (size_t)cur;
            const uint4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
            int k0, k1, k2, k3, r0, r1, r2, r3;
            quad_order(n0, n1, n2, n3, org, inv, s.bound * cscale, k0, k1, k2, k3, r0, r1, r2, r3);
            if (quad_descend(k0, k1, k2, k3, r0, r1, r2, r3, cur, [&](int ref) { stack[sp * 64] = ref; sp++; })) continue;
        } else {
            const int code = ~cur;
            int first = code >> 3, cnt = code & 7;
            while (cnt > 0) { tri_hits_pairrec<BOTH>(sc, first, cnt > 1, org, dir, inv, degenerate, s); first += 2; cnt -= 2; }
            if constexpr (SINK::kStops) { if (s.done()) return; }
        }
        if (sp == 0) return;
        sp--;
        cur = stack[sp * 64];
    }
}

// The walk over the binary tree, for a scene whose 4-wide walk would not fit kQueryStack (or PTAMD_QUERY_QUAD=0): trace_closest's
// control flow (pt_trace.h) — leaves tested on the spot, an entry pushed only where both children are interior: at most
// depth - 1 <= 31 entries — with the sink's bound in cullB.
template <bool BOTH, class SINK>
PT_DEV void hits_walk_binary(const DevScene& sc, const f3& org, const f3& dir, int* stack, SINK& s)
{
    const f3 inv(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
    const float L = __builtin_sqrtf(inv.x * inv.x + inv.y * inv.y + inv.z * inv.z);
    const f3 invD = inv / L;
    const bool degenerate = !(L < __builtin_inff());
    const float kcull = degenerate ? 1.0078125f : 1.0078125f / L;
    float cullB = s.bound * kcull;
    int sp = 0, cur = 0;
    for (;;) {
        if constexpr (SINK::kStops) { if (s.done()) return; }
        const float4 q0 = sc.nodes[4 * (size_t)cur + 0], q1 = sc.nodes[4 * (size_t)cur + 1], q2 = sc.nodes[4 * (size_t)cur + 2], q3 = sc.nodes[4 * (size_t)cur + 3];
        float tnL, tnR;
        bool okL, okR;
        if (!degenerate) {
            okL = box_test(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, org, invD, cullB, tnL);
            okR = box_test(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, org, invD, cullB, tnR);
        } else {
            okL = box_test_robust(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, org, dir, inv, cullB, tnL);
            okR = box_test_robust(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, org, dir, inv, cullB, tnR);
        }
        const int refL = __float_as_int(q3.x), refR = __float_as_int(q3.y);
        if (okL && refL < 0) {
            const int code = ~refL, first = code >> 3, cnt = code & 7;
            for (int k = 0; k < cnt; k++) tri_hits<BOTH>(sc, first + k, org, dir, invD, degenerate, s);
            cullB = s.bound * kcull;
            okL = false;
        }
        if (okR && refR < 0) {
            if (tnR <= cullB) {      // against what the left leaf left
                const int code = ~refR, first = code >> 3, cnt = code & 7;
                for (int k = 0; k < cnt; k++) tri_hits<BOTH>(sc, first + k, org, dir, invD, degenerate, s);
                cullB = s.bound * kcull;
            }
            okR = false;
        }
        if (okL & okR) {
            const bool lNear = tnL <= tnR;
            stack[sp * 64] = lNear ? refR : refL;
            sp++;
            cur = lNear ? refL : refR;
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

// The spheres, in order, after the walk: sphere_root's values (pt_trace.h), both roots kept apart.  Front: the one root Sphere::hit
// returns for [0, tmax].  Both sides: r1 if valid, and r2 if valid and not r1 again (r1 <= r2: the list takes them in that order).
template <bool BOTH, class SINK>
PT_DEV void sphere_hits(const DevScene& sc, const f3& org, const f3& dir, float tmax, SINK& s)
{
    for (int j = 0; j < sc.n_spheres; j++) {
        const float4 c = sc.spheres[4 * j];
        const f3 oc = org - f3(c.x, c.y, c.z);
        const float a = sqlen(dir);
        const float half_b = dot(oc, dir);
        const float cc = sqlen(oc) - c.w * c.w;
        const float disc = half_b * half_b - a * cc;
        if (disc < 0.f) continue;
        const float sq = __builtin_sqrtf(disc);
        const float r1 = (-half_b - sq) / a, r2 = (-half_b + sq) / a;
        const bool v1 = !(r1 < 0.f) & !(tmax < r1), v2 = !(r2 < 0.f) & !(tmax < r2);
        const int prim = sc.n_tris + j;
        if (BOTH) {
            if (v1 && s.wants(r1, prim)) s.take(r1, prim);
            if (v2 && r2 != r1 && s.wants(r2, prim)) s.take(r2, prim);
        } else {
            const float r = v1 ? r1 : r2;
            if ((v1 | v2) && s.wants(r, prim)) s.take(r, prim);
        }
    }
}

template <bool QUAD, bool BOTH, class SINK>
PT_DEV void hits_ray(const DevScene& sc, const f3& org, const f3& dir, float tmax, int* stack, SINK& s)
{
    if (QUAD) hits_walk_quad<BOTH>(sc, org, dir, stack, s);
    else hits_walk_binary<BOTH>(sc, org, dir, stack, s);
    sphere_hits<BOTH>(sc, org, dir, tmax, s);
}

// KC: the capacity class of the list (pt_scene.h: pt_kc_dispatch).  The wave's 64 rays own the 64 * k consecutive records from
// out[blockIdx.x * 64 * k]; every lane pads its list with miss records and the wave copies the block
// out of LDS in record order, 64 consecutive records (512 bytes) per store, exactly as nearest_k's points do.
// No waves-per-SIMD figure in the launch bounds, as in nearest_k: above KC = 4 the list's LDS, not the registers, decides how many
// workgroups a CU holds (DESIGN.md section 34 has the table; the registers allow kQueryWaves in every instantiation).
template <int KC, bool QUAD, bool BOTH>
__global__ __launch_bounds__(64)
void rays_k(DevScene sc, const float4* __restrict__ rays, uint32_t n, int k, int2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[KC * kSlotRow];
    if (k < 1 || k > KC) return;      // the launcher's choice of KC, restated where the list is indexed
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, i = base + lane;
    int2* list = &lds_list[lane];
    int cnt = 0;
    if (i < n) {
        f3 org, dir; float tmax;
        load_ray(rays, i, org, dir, tmax);
        SlotList<true> s{list, k, 0, tmax, -1};
        hits_ray<QUAD, BOTH>(sc, org, dir, tmax, &lds_stack[lane], s);
        cnt = s.cnt;
    }
    for (int j = cnt; j < k; j++) list[j * kSlotRow] = make_int2(0, -1);      // a miss is (0, -1)
    __syncthreads();
    const uint32_t live = (n - base < 64u) ? n - base : 64u, total = live * (uint32_t)k;
    int2* dst = out + (size_t)base * (size_t)k;
    const int q64 = 64 / k, m64 = 64 % k;
    int t = (int)lane / k, j = (int)lane % k;      // record r is slot j of ray t: r = t * k + j, t < live <= 64
    for (uint32_t r = lane; r < total; r += 64u) {
        dst[r] = lds_list[j * kSlotRow + t];
        j += m64;
        t += q64;
        if (j >= k) { j -= k; t++; }
    }
}

template <bool QUAD, bool BOTH>
__global__ __launch_bounds__(64, kQueryWaves)
void count_hits(DevScene sc, const float4* __restrict__ rays, uint32_t n, int32_t* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    f3 org, dir; float tmax;
    load_ray(rays, i, org, dir, tmax);
    HitCount s{0, tmax};
    hits_ray<QUAD, BOTH>(sc, org, dir, tmax, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// The 4-float detail record of the header for every finished slot, one thread per slot; zeros for a miss slot.  Slot t belongs to
// ray t / k.  A triangle is read from its surface record (indexed by primitive in the reference's order), which starts with V0 E1 E2,
// the floats its tri record holds.  Facing: a triangle was taken as a back face iff det < kEps; a sphere slot holds the entering
// root iff r1 is valid and is the slot's t (r2 is only ever kept beside a valid r1 when it differs from it).
// hit_detail: the record of a member h (h.y >= 0) of the ray's H, for rays_k_detail and rays_list_detail.
PT_DEV void hit_detail(const DevScene& sc, const f3& org, const f3& dir, float tmax, int2 h, float* o)
{
    const int prim = h.y;
    if (prim >= sc.n_tris) {
        const float4 c = sc.spheres[4 * (prim - sc.n_tris)];
        const f3 oc = org - f3(c.x, c.y, c.z);
        const float a = sqlen(dir);
        const float half_b = dot(oc, dir);
        const float cc = sqlen(oc) - c.w * c.w;
        const float disc = half_b * half_b - a * cc;
        const float r1 = (-half_b - __builtin_sqrtf(disc)) / a;
        const bool entering = !(r1 < 0.f) & !(tmax < r1) & (r1 == __int_as_float(h.x));
        o[0] = 0.f; o[1] = 0.f; o[2] = entering ? 1.f : -1.f; o[3] = 0.f;
        return;
    }
    const float4* rec = sc.surf + 12 * (size_t)prim;
    const float4 s0 = rec[0], s1 = rec[1], s2 = rec[2];
    const f3 V0(s0.x, s0.y, s0.z), E1(s0.w, s1.x, s1.y), E2(s1.z, s1.w, s2.x);
    const f3 T = org - V0;
    const f3 P = cross(dir, E2);
    const f3 Q = cross(T, E1);
    const float det = dot(P, E1);
    const float invDet = 1.f / det;
    o[0] = dot(P, T) * invDet; o[1] = dot(Q, dir) * invDet; o[2] = (det < kEps) ? -1.f : 1.f; o[3] = 0.f;
}

// A launch covers the slots from `first` on (pt_scene.h: pt_detail_chunks).
__global__ __launch_bounds__(256)
void rays_k_detail(DevScene sc, const float4* __restrict__ rays, uint64_t first, uint64_t slots, uint32_t k, const int2* __restrict__ res, float* __restrict__ out4)
{
    const uint64_t t = first + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= slots) return;
    const int2 h = res[t];
    const int prim = h.y;
    float* o = out4 + t * 4;      // 4-byte aligned: four stores
    if (prim < 0) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; return; }
    f3 org, dir; float tmax;
    load_ray(rays, t / k, org, dir, tmax);
    hit_detail(sc, org, dir, tmax, h, o);
}

// ---- every hit: the fill of pt_trace_rays_list (pt_lists.h says which code sorts which segment) ----------------
// One ray per lane, rays_k's shape with the list of class kListLds and the sink SlotSeg, whose long segments take HitCount's members.
// A lane whose segment is empty walks nothing.  Nothing outside [0, cap) is written: list_segment clamps.
template <bool QUAD, bool BOTH>
__global__ __launch_bounds__(64)
void rays_list(DevScene sc, const float4* __restrict__ rays, uint32_t n, const int64_t* __restrict__ off, int64_t cap, int2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kSlotRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t m = e - b;
    if (m == 0) return;
    f3 org, dir; float tmax;
    load_ray(rays, i, org, dir, tmax);
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    SlotSeg<true, HitCount> s(list, dst, m, tmax);
    hits_ray<QUAD, BOTH>(sc, org, dir, tmax, &lds_stack[lane], s);
    fill_write_out(list, dst, m, s.cnt, s.append);
}

// The detail records of every segment, after the sort: hit_detail per member slot (pt_lists.h: segments_detail)
__global__ __launch_bounds__(kSegThreads)
void rays_list_detail(DevScene sc, const float4* __restrict__ rays, uint32_t n, uint32_t per, const int64_t* __restrict__ off, int64_t cap,
                      const int2* __restrict__ res, float* __restrict__ out4)
{
    struct Ray { f3 org, dir; float tmax; };
    segments_detail<4>(off, n, per, cap, res, out4,
                       [&](uint32_t i) { Ray r; load_ray(rays, i, r.org, r.dir, r.tmax); return r; },
                       [&](const Ray& r, int2 h, float* o) { hit_detail(sc, r.org, r.dir, r.tmax, h, o); });
}

// ---- the filtered forms (include/pt_api.h: "Query filters") ----------------------------------------------------
// The kernels above with their sink behind pt_lists.h's Filtered: the same walks, the same one-wave workgroups and LDS layouts, the
// same capacity classes.  The ray's near bound is the 7th float of its record, which no other kernel reads.
PT_DEV LaneFilter load_ray_f(const float4* __restrict__ rays, uint32_t i, const QFilter& flt, f3& org, f3& dir, float& tmax)
{
    load_ray(rays, i, org, dir, tmax);
    return lane_filter(flt, i, rays[2 * (size_t)i + 1].z);      // the float4 load_ray has just fetched
}

// pt_trace_rays_f: the first member of H' under PT_HITS_FRONT, or (ANY) some member.  query_rays' shape and record.
template <bool ANY, bool QUAD>
__global__ __launch_bounds__(64, kQueryWaves)
void rays_one_f(DevScene sc, const float4* __restrict__ rays, uint32_t n, QFilter flt, float2* __restrict__ hits)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    f3 org, dir; float tmax;
    const LaneFilter lf = load_ray_f(rays, i, flt, org, dir, tmax);
    Filtered<SlotOne<ANY>> s{{tmax, -1, 0.f, -1}, lf};
    hits_ray<QUAD, false>(sc, org, dir, tmax, &lds_stack[threadIdx.x], s);
    hits[i] = make_float2(s.key, __int_as_float(s.prim));      // a miss is (0, -1)
}

template <int KC, bool QUAD, bool BOTH>
__global__ __launch_bounds__(64)
void rays_k_f(DevScene sc, const float4* __restrict__ rays, uint32_t n, int k, QFilter flt, int2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[KC * kSlotRow];
    if (k < 1 || k > KC) return;      // the launcher's choice of KC, restated where the list is indexed
    const uint32_t lane = threadIdx.x, base = blockIdx.x * 64u, i = base + lane;
    int2* list = &lds_list[lane];
    int cnt = 0;
    if (i < n) {
        f3 org, dir; float tmax;
        const LaneFilter lf = load_ray_f(rays, i, flt, org, dir, tmax);
        Filtered<SlotList<true>> s{{list, k, 0, tmax, -1}, lf};
        hits_ray<QUAD, BOTH>(sc, org, dir, tmax, &lds_stack[lane], s);
        cnt = s.cnt;
    }
    for (int j = cnt; j < k; j++) list[j * kSlotRow] = make_int2(0, -1);      // a miss is (0, -1)
    __syncthreads();
    klist_copy_out(lds_list, out, base, n, k);
}

template <bool QUAD, bool BOTH>
__global__ __launch_bounds__(64, kQueryWaves)
void count_hits_f(DevScene sc, const float4* __restrict__ rays, uint32_t n, QFilter flt, int32_t* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    f3 org, dir; float tmax;
    const LaneFilter lf = load_ray_f(rays, i, flt, org, dir, tmax);
    Filtered<HitCount> s{{0, tmax}, lf};
    hits_ray<QUAD, BOTH>(sc, org, dir, tmax, &lds_stack[threadIdx.x], s);
    out[i] = s.cnt;
}

// The fill: a long segment's appended members are Filtered<HitCount>'s members, the filtered count's
template <bool QUAD, bool BOTH>
__global__ __launch_bounds__(64)
void rays_list_f(DevScene sc, const float4* __restrict__ rays, uint32_t n, QFilter flt, const int64_t* __restrict__ off, int64_t cap,
                 int2* __restrict__ out)
{
    __shared__ int lds_stack[(QUAD ? kQueryStack : kStackDepth) * 64];
    __shared__ int2 lds_list[kListLds * kSlotRow];
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int64_t b, e;
    list_segment(off, i, cap, b, e);
    const int64_t m = e - b;
    if (m == 0) return;
    f3 org, dir; float tmax;
    const LaneFilter lf = load_ray_f(rays, i, flt, org, dir, tmax);
    int2* list = &lds_list[lane];
    int2* dst = out + b;
    Filtered<SlotSeg<true, HitCount>> s{SlotSeg<true, HitCount>(list, dst, m, tmax), lf};
    hits_ray<QUAD, BOTH>(sc, org, dir, tmax, &lds_stack[lane], s);
    fill_write_out(list, dst, m, s.cnt, s.append);
}

}  // namespace ptd

// f(std::bool_constant<QUAD>(), std::bool_constant<BOTH>()): the walk and the sides of a launch as compile-time values
template <class F>
static void quad_both_dispatch(bool quad, bool both, F f)
{
    if (quad) { if (both) f(std::true_type(), std::true_type()); else f(std::true_type(), std::false_type()); }
    else { if (both) f(std::false_type(), std::true_type()); else f(std::false_type(), std::false_type()); }
}

// Enqueues one batch of n <= 2^30 rays on `stream`: k records per ray, then the detail records if asked for
static hipError_t launch_rays_k(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, int k, bool quad, bool both, PtRayHit* d_hits, float* d_detail4, hipStream_t stream)
{
    const float4* rays = (const float4*)d_rays8;
    int2* out = (int2*)d_hits;
    const dim3 blocks((n + 63u) / 64u);
    pt_kc_dispatch(k, [&](auto kc) {
        if (quad) {
            if (both) hipLaunchKernelGGL((ptd::rays_k<kc, true, true>), blocks, dim3(64), 0, stream, sc, rays, n, k, out);
            else hipLaunchKernelGGL((ptd::rays_k<kc, true, false>), blocks, dim3(64), 0, stream, sc, rays, n, k, out);
        } else {
            if (both) hipLaunchKernelGGL((ptd::rays_k<kc, false, true>), blocks, dim3(64), 0, stream, sc, rays, n, k, out);
            else hipLaunchKernelGGL((ptd::rays_k<kc, false, false>), blocks, dim3(64), 0, stream, sc, rays, n, k, out);
        }
    });
    if (d_detail4)
        pt_detail_chunks((uint64_t)n * (uint64_t)k, [&](uint64_t first, dim3 grid) {
            hipLaunchKernelGGL(ptd::rays_k_detail, grid, dim3(256), 0, stream, sc, rays, first, (uint64_t)n * (uint64_t)k, (uint32_t)k, (const int2*)out, d_detail4);
        });
    return hipGetLastError();
}

static hipError_t launch_count_hits(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, bool quad, bool both, int32_t* d_count, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* rays = (const float4*)d_rays8;
    if (quad) {
        if (both) hipLaunchKernelGGL((ptd::count_hits<true, true>), blocks, dim3(64), 0, stream, sc, rays, n, d_count);
        else hipLaunchKernelGGL((ptd::count_hits<true, false>), blocks, dim3(64), 0, stream, sc, rays, n, d_count);
    } else {
        if (both) hipLaunchKernelGGL((ptd::count_hits<false, true>), blocks, dim3(64), 0, stream, sc, rays, n, d_count);
        else hipLaunchKernelGGL((ptd::count_hits<false, false>), blocks, dim3(64), 0, stream, sc, rays, n, d_count);
    }
    return hipGetLastError();
}

// Enqueues one batch of n <= 2^30 rays of pt_trace_rays_list on `stream`: the fill, the sort of the segments longer than kListLds,
// then the detail records if asked for.  off: the batch's first offset; the records are addressed from d_hits whatever the batch.
static hipError_t launch_rays_list(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, bool quad, bool both, const int64_t* off, int64_t cap,
                                   PtRayHit* d_hits, float* d_detail4, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* rays = (const float4*)d_rays8;
    int2* out = (int2*)d_hits;
    if (quad) {
        if (both) hipLaunchKernelGGL((ptd::rays_list<true, true>), blocks, dim3(64), 0, stream, sc, rays, n, off, cap, out);
        else hipLaunchKernelGGL((ptd::rays_list<true, false>), blocks, dim3(64), 0, stream, sc, rays, n, off, cap, out);
    } else {
        if (both) hipLaunchKernelGGL((ptd::rays_list<false, true>), blocks, dim3(64), 0, stream, sc, rays, n, off, cap, out);
        else hipLaunchKernelGGL((ptd::rays_list<false, false>), blocks, dim3(64), 0, stream, sc, rays, n, off, cap, out);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = ptk_list_sort(off, n, cap, out, true, stream)) != hipSuccess) return e;
    if (d_detail4) {
        uint32_t per, grid;
        pt_list_grid(n, per, grid);
        hipLaunchKernelGGL(ptd::rays_list_detail, dim3(grid), dim3(ptd::kSegThreads), 0, stream, sc, rays, n, per, off, cap, (const int2*)out, d_detail4);
    }
    return hipGetLastError();
}

// ---- the filtered forms' launchers: as the ones above, over the _f kernels ---------------------------------------------------------
hipError_t ptk_rays_one_f(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, bool any, bool quad, const ptd::QFilter& flt, PtRayHit* d_hits,
                          hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* rays = (const float4*)d_rays8;
    float2* hits = (float2*)d_hits;
    quad_both_dispatch(quad, any, [&](auto q, auto a) {
        hipLaunchKernelGGL((ptd::rays_one_f<decltype(a)::value, decltype(q)::value>), blocks, dim3(64), 0, stream, sc, rays, n, flt, hits);
    });
    return hipGetLastError();
}

static hipError_t launch_rays_k_f(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, int k, bool quad, bool both, const ptd::QFilter& flt,
                                  PtRayHit* d_hits, float* d_detail4, hipStream_t stream)
{
    const float4* rays = (const float4*)d_rays8;
    int2* out = (int2*)d_hits;
    const dim3 blocks((n + 63u) / 64u);
    pt_kc_dispatch(k, [&](auto kc) {
        quad_both_dispatch(quad, both, [&](auto q, auto b) {
            hipLaunchKernelGGL((ptd::rays_k_f<decltype(kc)::value, decltype(q)::value, decltype(b)::value>), blocks, dim3(64), 0, stream, sc, rays, n, k, flt, out);
        });
    });
    if (d_detail4)
        pt_detail_chunks((uint64_t)n * (uint64_t)k, [&](uint64_t first, dim3 grid) {
            hipLaunchKernelGGL(ptd::rays_k_detail, grid, dim3(256), 0, stream, sc, rays, first, (uint64_t)n * (uint64_t)k, (uint32_t)k, (const int2*)out, d_detail4);
        });
    return hipGetLastError();
}

static hipError_t launch_count_hits_f(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, bool quad, bool both, const ptd::QFilter& flt,
                                      int32_t* d_count, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* rays = (const float4*)d_rays8;
    quad_both_dispatch(quad, both, [&](auto q, auto b) {
        hipLaunchKernelGGL((ptd::count_hits_f<decltype(q)::value, decltype(b)::value>), blocks, dim3(64), 0, stream, sc, rays, n, flt, d_count);
    });
    return hipGetLastError();
}

static hipError_t launch_rays_list_f(const ptd::DevScene& sc, const float* d_rays8, uint32_t n, bool quad, bool both, const ptd::QFilter& flt,
                                     const int64_t* off, int64_t cap, PtRayHit* d_hits, float* d_detail4, hipStream_t stream)
{
    const dim3 blocks((n + 63u) / 64u);
    const float4* rays = (const float4*)d_rays8;
    int2* out = (int2*)d_hits;
    quad_both_dispatch(quad, both, [&](auto q, auto b) {
        hipLaunchKernelGGL((ptd::rays_list_f<decltype(q)::value, decltype(b)::value>), blocks, dim3(64), 0, stream, sc, rays, n, flt, off, cap, out);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = ptk_list_sort(off, n, cap, out, true, stream)) != hipSuccess) return e;
    if (d_detail4) {
        uint32_t per, grid;
        pt_list_grid(n, per, grid);
        hipLaunchKernelGGL(ptd::rays_list_detail, dim3(grid), dim3(ptd::kSegThreads), 0, stream, sc, rays, n, per, off, cap, (const int2*)out, d_detail4);
    }
    return hipGetLastError();
}

// ---- entry points (include/pt_api.h): every argument check comes before the first HIP call ----------------------------------------
static const char* flags_bad(int32_t flags)
{
    return (flags != PT_HITS_FRONT && flags != PT_HITS_BOTH_SIDES) ? "flags must be PT_HITS_FRONT or PT_HITS_BOTH_SIDES" : nullptr;
}

// has_k: pt_trace_rays_k and its host variant (PtRayHit records), else the counts
static int hits_args_ok(const char* who, const PtScene* s, const float* rays, int64_t n, bool has_k, int32_t k, int32_t flags, const void* out,
                        const float* detail, bool device, const PtQueryFilter* filter = nullptr)
{
    const char* param = (has_k && (k < 1 || k > PT_RAY_HITS_KMAX)) ? "k must be in 1 .. PT_RAY_HITS_KMAX" : flags_bad(flags);
    return pt_query_args(who, s, n, device, {"rays", rays, "out", out, has_k ? "hits" : "count", has_k ? 8 : 4, "detail", detail, param, false, nullptr, 0,
                                                   filter, true});
}

// pt_trace_rays_list and its host variant
static int list_args_ok(const char* who, const PtScene* s, const float* rays, int64_t n, int32_t flags, const int64_t* offsets, int64_t cap,
                        const void* hits, const float* detail, bool device, const PtQueryFilter* filter = nullptr)
{
    return pt_query_args(who, s, n, device, {"rays", rays, "hits", hits, "hits", 8, "detail", detail, flags_bad(flags), true, offsets, cap, filter, true});
}

extern "C" {

int pt_trace_rays_k(PtScene* s, const float* d_rays8, int64_t n, int32_t k, int32_t flags, PtRayHit* d_hits, float* d_detail4, void* hip_stream)
{
    int rc;
    if ((rc = hits_args_ok("pt_trace_rays_k", s, d_rays8, n, true, k, flags, d_hits, d_detail4, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s), both = flags == PT_HITS_BOTH_SIDES;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_rays_k(s->dev, d_rays8 + off * 8, m, k, quad, both, d_hits + off * k, d_detail4 ? d_detail4 + off * k * 4 : nullptr, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_trace_rays_k_host(PtScene* s, const float* h_rays8, int64_t n, int32_t k, int32_t flags, PtRayHit* h_hits, float* h_detail4)
{
    int rc;
    if ((rc = hits_args_ok("pt_trace_rays_k_host", s, h_rays8, n, true, k, flags, h_hits, h_detail4, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const size_t slots = (size_t)n * (size_t)k;
    return pt_host_query(h_rays8, (size_t)n * 32, h_hits, slots * 8, h_detail4, slots * 16, [&](float* d_rays, void* d_hits, float* d_det) {
        return pt_trace_rays_k(s, d_rays, n, k, flags, (PtRayHit*)d_hits, d_det, nullptr);
    });
}

int pt_count_hits(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, int32_t* d_count, void* hip_stream)
{
    int rc;
    if ((rc = hits_args_ok("pt_count_hits", s, d_rays8, n, false, 0, flags, d_count, nullptr, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s), both = flags == PT_HITS_BOTH_SIDES;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_count_hits(s->dev, d_rays8 + off * 8, m, quad, both, d_count + off, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_count_hits_host(PtScene* s, const float* h_rays8, int64_t n, int32_t flags, int32_t* h_count)
{
    int rc;
    if ((rc = hits_args_ok("pt_count_hits_host", s, h_rays8, n, false, 0, flags, h_count, nullptr, false)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    return pt_host_query(h_rays8, (size_t)n * 32, h_count, (size_t)n * 4, nullptr, 0, [&](float* d_rays, void* d_count, float*) {
        return pt_count_hits(s, d_rays, n, flags, (int32_t*)d_count, nullptr);
    });
}

int pt_trace_rays_list(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, const int64_t* d_offsets, int64_t cap, PtRayHit* d_hits,
                       float* d_detail4, void* hip_stream)
{
    int rc;
    if ((rc = list_args_ok("pt_trace_rays_list", s, d_rays8, n, flags, d_offsets, cap, d_hits, d_detail4, true)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s), both = flags == PT_HITS_BOTH_SIDES;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_rays_list(s->dev, d_rays8 + off * 8, m, quad, both, d_offsets + off, cap, d_hits, d_detail4, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_trace_rays_list_host(PtScene* s, const float* h_rays8, int64_t n, int32_t flags, int64_t* h_offsets, int64_t cap, PtRayHit* h_hits,
                            float* h_detail4)
{
    int rc;
    if ((rc = list_args_ok("pt_trace_rays_list_host", s, h_rays8, n, flags, h_offsets, cap, h_hits, h_detail4, false)) != PT_OK) return rc;
    if (n == 0) { h_offsets[0] = 0; return PT_OK; }
    HIPCHK(hipSetDevice(s->device));
    return pt_host_list("pt_trace_rays_list_host", h_rays8, n, 32, h_offsets, cap, h_hits, h_detail4, 16,
                        [&](float* d_rays, int32_t* d_count) { return pt_count_hits(s, d_rays, n, flags, d_count, nullptr); },
                        [&](float* d_rays, int64_t* d_off, int64_t total, void* d_hits, float* d_det) {
                            return pt_trace_rays_list(s, d_rays, n, flags, d_off, total, (PtRayHit*)d_hits, d_det, nullptr);
                        });
}

// ---- the filtered forms: the twin's checks, then the filter's; a neutral filter enqueues the twin itself ---------------------------
int pt_trace_rays_k_f(PtScene* s, const float* d_rays8, int64_t n, int32_t k, int32_t flags, const PtQueryFilter* filter, PtRayHit* d_hits,
                      float* d_detail4, void* hip_stream)
{
    int rc;
    if ((rc = hits_args_ok("pt_trace_rays_k_f", s, d_rays8, n, true, k, flags, d_hits, d_detail4, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_trace_rays_k(s, d_rays8, n, k, flags, d_hits, d_detail4, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s), both = flags == PT_HITS_BOTH_SIDES;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_rays_k_f(s->dev, d_rays8 + off * 8, m, k, quad, both, pt_filter_dev(filter, off), d_hits + off * k,
                               d_detail4 ? d_detail4 + off * k * 4 : nullptr, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_count_hits_f(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, const PtQueryFilter* filter, int32_t* d_count, void* hip_stream)
{
    int rc;
    if ((rc = hits_args_ok("pt_count_hits_f", s, d_rays8, n, false, 0, flags, d_count, nullptr, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_count_hits(s, d_rays8, n, flags, d_count, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s), both = flags == PT_HITS_BOTH_SIDES;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_count_hits_f(s->dev, d_rays8 + off * 8, m, quad, both, pt_filter_dev(filter, off), d_count + off, (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

int pt_trace_rays_list_f(PtScene* s, const float* d_rays8, int64_t n, int32_t flags, const int64_t* d_offsets, int64_t cap, const PtQueryFilter* filter,
                         PtRayHit* d_hits, float* d_detail4, void* hip_stream)
{
    int rc;
    if ((rc = list_args_ok("pt_trace_rays_list_f", s, d_rays8, n, flags, d_offsets, cap, d_hits, d_detail4, true, filter)) != PT_OK) return rc;
    if (n == 0) return PT_OK;
    if (pt_filter_neutral(filter)) return pt_trace_rays_list(s, d_rays8, n, flags, d_offsets, cap, d_hits, d_detail4, hip_stream);
    HIPCHK(hipSetDevice(s->device));
    const bool quad = pt_query_walks_quad(s), both = flags == PT_HITS_BOTH_SIDES;
    HIPCHK(pt_query_batches(n, [&](int64_t off, uint32_t m) {
        return launch_rays_list_f(s->dev, d_rays8 + off * 8, m, quad, both, pt_filter_dev(filter, off), d_offsets + off, cap, d_hits, d_detail4,
                                  (hipStream_t)hip_stream);
    }));
    return PT_OK;
}

}  // extern "C"

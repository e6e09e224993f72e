"""CPU models of the two in-kernel margins that DESIGN.md section 31 left open: the 2^-20 widening of quad_order (csrc/pt_trace.h) and the
margin of shadow_stop_t (csrc/pt_stream.h).  Pure numpy, float32 operation for operation: every numpy float32 operation rounds once, as
the device's do (no contraction, correctly rounded divide and sqrt), and the one fused operation, fmaf, is computed exactly (fma32).
tests/test_slack.py holds quad_child_accepts and binary_child_accepts against the kernels' own functions compiled for the host, bit for bit.

A traversal tree only steers the search: a triangle the reference accepts is found iff every box on the way from the root to its leaf (its
chain) lets the ray through.  needed_slack is the least widening of quad_order at which the whole chain does."""
import numpy as np

F = np.float32
D = np.float64
K_SL = 2.0 ** -20                   # quad_order's kSl
K_CSCALE = F(1.0000019)             # ray_setup: cscale = rcp(L) * 1.0000019f
K_FAR = F(1.00000024)               # box_test: the reference's scaling of the far side
K_CULL = F(1.0078125)               # trace_closest: kcull = 1.0078125f / L
SHADOW_FLOOR, SHADOW_ULPS = F(5e-4), F(7.6293945e-6)      # shadow_stop_t: max(5e-4, mag * 2^-17)
EPS = F(1e-4)                       # the reference's EPS (kEps)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded, where a * b is exact in float64 (here a is a byte, 0 .. 255).  The sum is
    formed in float64 with its rounding error (two-sum); rounding that sum to float32 differs from rounding the exact value only when
    the float64 sum lies exactly half way between two float32 values and the error is not 0: the error then decides the direction."""
    a, b, c = (np.asarray(x, F).astype(D) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(F)
        rd = r.astype(D)
        up, dn = np.nextafter(r, F(np.inf)).astype(D), np.nextafter(r, F(-np.inf)).astype(D)
        fin = np.isfinite(s) & np.isfinite(up) & np.isfinite(dn)
        tie_up = fin & (s > rd) & ((s - rd) == (up - s)) & (err > 0)
        tie_dn = fin & (s < rd) & ((rd - s) == (s - dn)) & (err < 0)
    return np.where(tie_up, up, np.where(tie_dn, dn, rd)).astype(F)


def ray_setup(d, worst_rcp=True):
    """ray_setup of csrc/pt_trace.h for non-degenerate directions (n, 3): (inv, cscale, degenerate).  inv = Normalize(1 / dir).  The device
    forms cscale with an approximate reciprocal; worst_rcp models the smallest it can be, the exact 1 / L rounded down, times 1.0000019
    (the cull then bites earliest); worst_rcp = False rounds 1 / L to nearest."""
    d = np.asarray(d, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F(1) / d
        L = np.sqrt((inv[:, 0] * inv[:, 0] + inv[:, 1] * inv[:, 1]) + inv[:, 2] * inv[:, 2])
        deg = ~(L < F(np.inf))
        invn = inv / L[:, None]
        r = D(1) / L.astype(D)
        r32 = r.astype(F)
        if worst_rcp:
            r32 = np.where(r32.astype(D) > r, np.nextafter(r32, F(-np.inf)), r32)      # 1 / L is never a float32 tie: rounded down
        cscale = (r32 * K_CSCALE).astype(F)
    return invn.astype(F), cscale, deg


def quad_child_accepts(quad, node, k, org, inv, cullT, slack=K_SL):
    """quad_order's test of child k (0 .. 3) of 4-wide node `node`, for rays (org, inv) (n, 3) with the cull distance cullT (n,) in the
    walk's units: True where key[k] != kQuadMiss.  node and k may be arrays (one per ray).  Returns (accepts, tn)."""
    q = np.ascontiguousarray(quad, np.uint32).reshape(-1, 16)
    org, inv = np.asarray(org, F), np.asarray(inv, F)
    n = len(org)
    node = np.broadcast_to(np.asarray(node, np.int64), (n,))
    k = np.broadcast_to(np.asarray(k, np.int64), (n,))
    rec = q[node]                                                   # (n, 16)
    recf = rec.view(F)
    sl = np.broadcast_to(np.asarray(slack, F), (n,))              # one value, or one per ray
    shift = (8 * k).astype(np.uint32)
    tn_ax, tf_ax = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for a, (sc_col, lo_col, hi_col) in enumerate(((3, 8, 11), (14, 9, 12), (15, 10, 13))):
            A = inv[:, a] * recf[:, sc_col]
            B = (recf[:, a] - org[:, a]) * inv[:, a]
            s = (np.abs(B) + F(255) * np.abs(A)) * sl
            Bn, Bf = B - s, B + s
            neg = (inv[:, a].view(np.int32) >> 31) != 0             # the sign bit, -0 included
            lo, hi = rec[:, lo_col], rec[:, hi_col]
            nq = ((np.where(neg, hi, lo) >> shift) & np.uint32(255)).astype(F)
            fq = ((np.where(neg, lo, hi) >> shift) & np.uint32(255)).astype(F)
            tn_ax.append(fma32(nq, A, Bn))
            tf_ax.append(fma32(fq, A, Bf))
        tn = np.fmax(np.fmax(tn_ax[0], tn_ax[1]), np.fmax(tn_ax[2], F(0)))
        tf = np.fmin(np.fmin(tf_ax[0], tf_ax[1]), np.fmin(tf_ax[2], np.asarray(cullT, F)))
        return tn <= tf, tn


def box_test(box6, org, invD, cullB):
    """box_test of csrc/pt_trace.h on boxes (n, 6) (bmin, bmax): (accepts, tn)."""
    b, org, invD = np.asarray(box6, F), np.asarray(org, F), np.asarray(invD, F)
    with np.errstate(invalid="ignore", over="ignore"):
        t1 = (b[:, 0:3] - org) * invD
        t2 = (b[:, 3:6] - org) * invD
        mn, mx = np.fmin(t1, t2), np.fmax(t1, t2)
        tn = np.fmax(mn[:, 2], np.fmax(mn[:, 1], np.fmax(mn[:, 0], F(0))))
        tf = np.fmin(mx[:, 2], np.fmin(mx[:, 1], mx[:, 0])) * K_FAR
        return (tn <= tf) & (tn <= np.asarray(cullB, F)), tn


def binary_child_accepts(nodes, node, side, org, invD, cullB):
    """trace_closest's box_test of child `side` (0 = L, 1 = R) of binary record `node` (`nodes`: 16 floats per record)."""
    rec = np.ascontiguousarray(nodes, F).reshape(-1, 16)
    n = len(org)
    node = np.broadcast_to(np.asarray(node, np.int64), (n,))
    side = np.broadcast_to(np.asarray(side, np.int64), (n,))
    r = rec[node]
    box = np.where((side == 0)[:, None], r[:, 0:6], r[:, 6:12])
    return box_test(box, org, invD, cullB)


def binary_cull(t, d):
    """trace_closest's cullB for a closest hit at t along non-degenerate directions d: t * (1.0078125f / L)."""
    d = np.asarray(d, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F(1) / d
        L = np.sqrt((inv[:, 0] * inv[:, 0] + inv[:, 1] * inv[:, 1]) + inv[:, 2] * inv[:, 2])
        return (np.asarray(t, F) * (K_CULL / L)).astype(F)


class Trees:
    """The five arrays of an upload (tools/dump_accel.cpp, or pt_dbg_scene_array) and, for every primitive (the reference's index,
    tri[:, 3]), its chains: the (node, slot) pairs from the root to the leaf that holds it, in the 4-wide tree and in the binary one."""

    def __init__(self, nodes, quad, tri, leafbox=None):
        self.nodes = np.ascontiguousarray(nodes, F).reshape(-1, 16)
        self.quad = np.ascontiguousarray(quad).view(np.uint32).reshape(-1, 16)
        self.tri = np.ascontiguousarray(tri, F).reshape(-1, 12)
        self.leafbox = None if leafbox is None else np.ascontiguousarray(leafbox, F).reshape(-1, 8)
        self.prim_of = self.tri[:, 3].view(np.int32).astype(np.int64)
        self.n = len(self.tri)
        self.quad_chain = self._chains(self.quad[:, 4:8].view(np.int32), 4)
        self.bin_chain = self._chains(self.nodes[:, 12:14].view(np.int32), 2)

    def _chains(self, refs, width):
        """(node (n_prims, depth), slot (n_prims, depth), length (n_prims,)), indexed by primitive; unused levels hold -1."""
        chains = [None] * self.n
        stack = [(0, [])]
        while stack:
            i, path = stack.pop()
            for k in range(width):
                ref = int(refs[i, k])
                if ref >= 0:
                    stack.append((ref, path + [(i, k)]))
                elif (~ref & 7) != 0:
                    first, cnt = (~ref) >> 3, (~ref) & 7
                    for qi in range(first, first + cnt):
                        assert chains[self.prim_of[qi]] is None, "a triangle is reached twice"
                        chains[self.prim_of[qi]] = path + [(i, k)]
        assert all(c is not None for c in chains), "a triangle is not reached"
        depth = max(len(c) for c in chains)
        node, slot = np.full((self.n, depth), -1, np.int64), np.full((self.n, depth), -1, np.int64)
        for p, c in enumerate(chains):
            node[p, :len(c)], slot[p, :len(c)] = [x[0] for x in c], [x[1] for x in c]
        return node, slot, np.array([len(c) for c in chains])

    def leaf_child_boxes(self):
        """(m, 6) float64 lo, hi of every child box of the 4-wide tree that is a leaf, decoded: origin + scale * q."""
        q = self.quad
        qf, refs = q.view(F), q[:, 4:8].view(np.int32)
        out = []
        for k in range(4):
            m = (refs[:, k] < 0) & ((~refs[:, k] & 7) != 0)
            org = qf[m][:, 0:3].astype(D)
            sc = np.stack([qf[m][:, 3], qf[m][:, 14], qf[m][:, 15]], 1).astype(D)
            lo = np.stack([(q[m][:, 8 + a] >> np.uint32(8 * k)) & np.uint32(255) for a in range(3)], 1).astype(D)
            hi = np.stack([(q[m][:, 11 + a] >> np.uint32(8 * k)) & np.uint32(255) for a in range(3)], 1).astype(D)
            out.append(np.concatenate([org + sc * lo, org + sc * hi], 1))
        return np.concatenate(out)


def chain_of(trees, prim, which="quad"):
    """The ancestor (node, slot) list from the root to the leaf holding primitive `prim`, in the 4-wide tree ("quad") or the binary one."""
    node, slot, ln = trees.quad_chain if which == "quad" else trees.bin_chain
    return [(int(node[prim, j]), int(slot[prim, j])) for j in range(int(ln[prim]))]


def quad_chain_accepts(trees, rays8, prim, t, slack=K_SL, worst_rcp=True):
    """True where every box on the 4-wide chain of prim[i] accepts ray i with the cull at the closest hit t[i] (the walk's bestT is never
    below it), quad_order widened by `slack` (a scalar, or one value per ray)."""
    rays8 = np.asarray(rays8, F)
    org, d = rays8[:, 0:3], rays8[:, 3:6]
    inv, cscale, deg = ray_setup(d, worst_rcp)
    cullT = (np.asarray(t, F) * cscale).astype(F)
    node, slot, ln = trees.quad_chain
    prim = np.asarray(prim, np.int64)
    ok = np.ones(len(rays8), bool)
    sl = np.broadcast_to(np.asarray(slack, F), (len(rays8),))
    for j in range(node.shape[1]):
        live = np.nonzero(ln[prim] > j)[0]
        if not len(live):
            break
        m = live
        acc, _ = quad_child_accepts(trees.quad, node[prim[m], j], slot[prim[m], j], org[m], inv[m], cullT[m], sl[m])
        ok[m] &= acc
    return ok | deg


def binary_chain_accepts(trees, rays8, prim, t):
    """The same for trace_closest's walk of the binary tree (it has no slack of its own: the far side is scaled by 1.00000024 and the cull
    by 1.0078125)."""
    rays8 = np.asarray(rays8, F)
    org, d = rays8[:, 0:3], rays8[:, 3:6]
    inv, _, deg = ray_setup(d)
    cullB = binary_cull(t, d)
    node, slot, ln = trees.bin_chain
    prim = np.asarray(prim, np.int64)
    ok = np.ones(len(rays8), bool)
    for j in range(node.shape[1]):
        m = np.nonzero(ln[prim] > j)[0]
        if not len(m):
            break
        acc, _ = binary_child_accepts(trees.nodes, node[prim[m], j], slot[prim[m], j], org[m], inv[m], cullB[m])
        ok[m] &= acc
    return ok | deg


def needed_slack(trees, rays8, prim, t, worst_rcp=True):
    """(n,) float32: the least slack of quad_order at which every box on prim's 4-wide chain accepts the ray, cullT from the closest hit t.
    0 where the chain accepts unwidened; inf where no slack up to 2^8 does.  Dyadic values 2^-40 .. 2^8 first, then bisection over the
    float32 values between the last refused and the first accepted power of two, to one float32 step."""
    rays8, prim, t = np.asarray(rays8, F), np.asarray(prim, np.int64), np.asarray(t, F)
    out = np.zeros(len(rays8), F)
    todo = np.nonzero(~quad_chain_accepts(trees, rays8, prim, t, 0.0, worst_rcp))[0]
    if not len(todo):
        return out
    out[todo] = F(np.inf)
    r, p, tt = rays8[todo], prim[todo], t[todo]
    first = np.full(len(todo), 99, np.int64)
    for e in range(-40, 9):
        m = np.nonzero(first == 99)[0]
        if not len(m):
            break
        acc = quad_chain_accepts(trees, r[m], p[m], tt[m], 2.0 ** e, worst_rcp)
        first[m[acc]] = e
    found = np.nonzero(first != 99)[0]
    if len(found):
        hi = np.ldexp(F(1), first[found].astype(np.int32)).astype(F).view(np.uint32).astype(np.int64)      # accepted
        lo = np.where(first[found] == -40, 0, hi - (1 << 23))                                              # refused (2^(e-1), or 0)
        while ((hi - lo) > 1).any():
            mid = (lo + hi) // 2
            acc = quad_chain_accepts(trees, r[found], p[found], tt[found], mid.astype(np.uint32).view(F), worst_rcp)
            go = (hi - lo) > 1
            hi = np.where(go & acc, mid, hi)
            lo = np.where(go & ~acc, mid, lo)
        out[todo[found]] = hi.astype(np.uint32).view(F)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the shadow ray's early stop
# ---------------------------------------------------------------------------------------------------------------------------------
def shadow_stop_margin(p, tmax):
    """The margin shadow_stop_t subtracts from tmax - 1 for a shadow ray from p (n, 3) with t_max tmax: max(5e-4, mag * 2^-17)."""
    p, tmax = np.asarray(p, F), np.asarray(tmax, F)
    mag = np.fmax(np.fmax(np.abs(p[:, 0]), np.abs(p[:, 1])), np.fmax(np.abs(p[:, 2]), tmax))
    return np.fmax(SHADOW_FLOOR, mag * SHADOW_ULPS)


def shadow_needed_margin(p, P, tmax, t_closest, lit):
    """For shadow rays from p to the light point P with t_max tmax = |P - p| + 1 whose closest hit lies at t_closest: where the reference's
    verdict is "visible" (lit), the margin below which wf_trace's early stop `bestT < stopBelow` would end the ray at that very hit and
    call it dark: (tmax - 1) - t_closest in float32, as the device forms tmax - 1.  The shipped margin must exceed it on every lit row
    (stopBelow = (tmax - 1) - margin <= t_closest).  NaN where the row is not lit."""
    tmax, t_closest = np.asarray(tmax, F), np.asarray(t_closest, F)
    need = (tmax - F(1)) - t_closest
    return np.where(np.asarray(lit, bool), need, F(np.nan)).astype(F)


VEIL_DISTANCES = tuple(x * 1e-4 for x in (0.25, 0.5, 0.9, 1.1, 2.0, 4.0, 6.0))      # in front of the light, in units of EPS
VEIL_LIGHT_Y, VEIL_HALF = 39.95, 5.0


def veil_emittance(k):
    return (3.0 + k, 20.0 - 2.0 * k, 1.0 + 3.0 * k)      # none is the light's (15, 15, 15)


def veil_scene(Dg, tr, make_prims, walls):
    """The Cornell room (`walls`: scenes_util._cornell_walls() records) with a 10 x 10 ceiling light of emittance 15 at y = 39.95, cut
    into 7 strips along x of 16 triangles each, and an emissive veil (2 triangles, veil_emittance(k)) VEIL_DISTANCES[k] below strip k.
    The room is placed by x * Dg + tr in float64 and rounded once; the veil distances are NOT scaled (the reference's EPS is absolute):
    a veil's height is the placed light's minus its distance, rounded to float32.  Returns ((n, 84) Primitive records, the patch
    centres (7, 3) float64 in home coordinates)."""
    Dg, tr = np.asarray(Dg, D), np.asarray(tr, D)
    wp = walls.reshape(len(walls), 3, 28)[:, :, 0:3].astype(D) * Dg + tr
    parts = [None]
    parts[0] = make_prims(wp[:, 0].astype(F), wp[:, 1].astype(F), wp[:, 2].astype(F), albedo=walls[:, 17:20])
    centres = []
    h, y = VEIL_HALF, VEIL_LIGHT_Y
    for k, dist in enumerate(VEIL_DISTANCES):
        x0, x1 = -h + 2 * h * k / 7.0, -h + 2 * h * (k + 1) / 7.0
        centres.append((0.5 * (x0 + x1), y, 0.0))
        zs = np.linspace(-h, h, 9)
        a, b, c = [], [], []
        for j in range(8):      # facing down: (x0,z0) (x1,z0) (x1,z1) has its normal along -y
            q = [(x0, y, zs[j]), (x1, y, zs[j]), (x1, y, zs[j + 1]), (x0, y, zs[j + 1])]
            a += [q[0], q[0]]; b += [q[1], q[2]]; c += [q[2], q[3]]
        a, b, c = (np.array(v, D) * Dg + tr for v in (a, b, c))
        parts.append(make_prims(a.astype(F), b.astype(F), c.astype(F), albedo=(0, 0, 0), emit=(15, 15, 15)))
        q = np.array([(x0, y, -h), (x1, y, -h), (x1, y, h), (x0, y, h)], D) * Dg + tr
        q[:, 1] -= dist
        q = q.astype(F)
        parts.append(make_prims(q[[0, 0]], q[[1, 2]], q[[2, 3]], albedo=(0, 0, 0), emit=veil_emittance(k)))
    return np.ascontiguousarray(np.concatenate(parts), F), np.array(centres, D)


def veil_rows(rs, centres, Dg, tr, per_patch=512):
    """o_nee / pt_dbg_nee rows (p.xyz, two seed words as float bits): surface points under each patch, 0.05 .. 30 home units from the
    patch centre at 0 .. 89 degrees from the light's normal (a quarter at normal incidence exactly), kept inside the room, and 64 far below it; placed."""
    out = []
    for c in centres:
        th = np.radians(rs.uniform(0, 89, per_patch))
        th[::4] = 0.0
        ph = rs.uniform(0, 2 * np.pi, per_patch)
        dist = 2.0 ** rs.uniform(np.log2(0.05), np.log2(30.0), per_patch)
        p = c + dist[:, None] * np.stack([np.sin(th) * np.cos(ph), -np.cos(th), np.sin(th) * np.sin(ph)], 1)
        out.append(np.clip(p, [-19.5, 0.5, -19.5], [19.5, 39.9, 19.5]))
        # ... and 64 points 600 .. 4000 units under the patch, within 2 degrees of the normal.  They see the light through the floor (its back
        # face is culled), t is in the thousands and one float32 step of t (6e-5 .. 2.4e-4) is itself more than half of EPS: where a float32
        # step of the coordinates is above every veil distance (far12, far17) these are the lit rows that need a margin at all.
        th = np.radians(rs.uniform(0, 2, 64))
        ph = rs.uniform(0, 2 * np.pi, 64)
        dist = 2.0 ** rs.uniform(np.log2(600.0), np.log2(4000.0), 64)
        out.append(c + dist[:, None] * np.stack([np.sin(th) * np.cos(ph), -np.cos(th), np.sin(th) * np.sin(ph)], 1))
    p = (np.concatenate(out) * np.asarray(Dg, D) + np.asarray(tr, D)).astype(F)
    seeds = rs.randint(0, 2 ** 32, (len(p), 2), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([p, seeds.view(F)], 1), F)


def shadow_ray(p, P):
    """The shadow ray GetLightColor casts from p to P (include/CudaUtil.cuh:150-166): RAY8 records with dir = Normalize(P - p) — the
    reference's Normalize divides every component by the length — and t_max = |P - p| + 1."""
    p, P = np.asarray(p, F), np.asarray(P, F)
    to = (P - p).astype(F)
    ln = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2])
    out = np.zeros((len(p), 8), F)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 0:3], out[:, 3:6], out[:, 7] = p, to / ln[:, None], ln + F(1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# adversarial ray families: candidates only; the oracle says which of them hit what, the model what they need
# ---------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _aim(org, tgt):
    """scenes_util._aim: RAY8 records from org to tgt, the direction (tgt - org) in float32 times a power of two."""
    org, tgt = np.asarray(org, F), np.asarray(tgt, F)
    d = (tgt - org).astype(F)
    e = np.frexp(np.abs(d).max(1))[1]
    d = np.ldexp(d, -e[:, None]).astype(F)
    n = len(org)
    return np.concatenate([org, d, np.zeros((n, 1), F), np.full((n, 1), 999999.0, F)], 1).astype(F)


def sliver_rays(rs, n, pos, idx, dist_lo, dist_hi):
    """Families (a) and (b): n RAY8 candidates at the long thin triangles idx of pos (m, 3, 3), and the triangle each is aimed at.
    Targets: along the longest edge from 0.3 edge lengths before one end to 0.3 past the other (a quarter each: before the first end,
    past the second, inside, anywhere) and across it from one width outside the long edge to one width past the apex; three in ten lie
    exactly on the long edge or on the line of one of the two other edges, +- 10^-3 of the width.  Origins: dist_lo .. dist_hi away
    (log-uniform) at an angle to the normal whose cosine is log-uniform from where det = |E1 x E2| cos reaches kEps (EPS = 10^-4; half of
    that, since _aim leaves |dir| in [0.5, 1.74)) up to 1; half of them within 0.02 rad of the plane through the normal and the long edge."""
    pick = np.asarray(idx)[rs.randint(0, len(idx), n)]
    v = np.asarray(pos, D)[pick]
    ed = np.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], v[:, 2] - v[:, 1]], 1)
    which = np.argmax((ed * ed).sum(2), 1)
    a = np.where((which == 2)[:, None], v[:, 1], v[:, 0])
    b = np.where((which == 0)[:, None], v[:, 1], v[:, 2])
    c = np.where((which == 0)[:, None], v[:, 2], np.where((which == 1)[:, None], v[:, 1], v[:, 0]))
    el = b - a
    cr = np.cross(ed[:, 0], ed[:, 1])
    area2 = np.sqrt((cr * cr).sum(1))
    nrm = cr / area2[:, None]
    u = _unit(el)
    w = np.cross(nrm, u)
    apex_w = ((c - a) * w).sum(1)
    apex_s = ((c - a) * u).sum(1) / np.sqrt((el * el).sum(1))
    kind = rs.randint(0, 4, n)
    s = np.select([kind == 0, kind == 1, kind == 2], [rs.uniform(-0.3, 0.02, n), rs.uniform(0.98, 1.3, n), rs.uniform(0, 1, n)], rs.uniform(-0.3, 1.3, n))
    ww = rs.uniform(-1.0, 2.0, n) * apex_w
    on_edge = np.where(s < apex_s, s / apex_s, (1 - s) / (1 - apex_s)) * apex_w
    exact = np.where(rs.uniform(0, 1, n) < 0.5, 0.0, on_edge) + apex_w * rs.uniform(-1e-3, 1e-3, n)
    ww = np.where(rs.uniform(0, 1, n) < 0.3, exact, ww)
    tgt = a + s[:, None] * el + ww[:, None] * w
    cmin = np.minimum(0.5 * float(EPS) / area2, 0.5)
    cth = np.exp(rs.uniform(0, 1, n) * np.log(cmin))
    sth = np.sqrt(1 - cth * cth)
    ph = rs.uniform(0, 2 * np.pi, n)
    ph = np.where(rs.uniform(0, 1, n) < 0.5, np.where(rs.uniform(0, 1, n) < 0.5, 0.0, np.pi) + rs.uniform(-0.02, 0.02, n), ph)
    off = cth[:, None] * nrm + sth[:, None] * (np.cos(ph)[:, None] * u + np.sin(ph)[:, None] * w)
    dist = 2.0 ** rs.uniform(np.log2(dist_lo), np.log2(dist_hi), n)
    return _aim((tgt + off * dist[:, None]).astype(F), tgt.astype(F)), pick


def corner_rays(rs, n, boxes, dist_lo, dist_hi):
    """Family (c): n RAY8 candidates grazing the corners, edges and faces of the boxes (m, 6) float64 (lo, hi; the decoded leaf child boxes
    of the 4-wide tree): the target is a corner (a half), a point on an edge (a quarter) or on a face, moved by up to 4 float32 steps of
    its largest coordinate in every axis (a fifth: not at all); the origin lies dist_lo .. dist_hi away (log-uniform) in a uniform direction."""
    bx = np.asarray(boxes, D)
    b = bx[rs.randint(0, len(bx), n)]
    f = rs.randint(0, 2, (n, 3)).astype(D)
    kind = rs.uniform(0, 1, n)
    free = np.where(kind < 0.5, 0, np.where(kind < 0.75, 1, 2))      # how many coordinates leave the corner
    ax = np.argsort(rs.uniform(0, 1, (n, 3)), 1)
    for j in range(2):
        m = free > j
        f[np.nonzero(m)[0], ax[m, j]] = rs.uniform(0, 1, int(m.sum()))
    tgt = b[:, 0:3] + f * (b[:, 3:6] - b[:, 0:3])
    step = np.spacing(np.abs(tgt).max(1).astype(F)).astype(D)
    tgt = tgt + np.where((rs.uniform(0, 1, n) < 0.2)[:, None], 0.0, rs.randint(-4, 5, (n, 3)) * step[:, None])
    d = _unit(rs.standard_normal((n, 3)))
    dist = 2.0 ** rs.uniform(np.log2(dist_lo), np.log2(dist_hi), n)
    return _aim((tgt + d * dist[:, None]).astype(F), tgt.astype(F))


def cluster_rays(rs, n, pos, idx, boxes, dist_lo, dist_hi):
    """Family (d): a large B over small boxes.  n RAY8 candidates at the small triangles idx of pos from dist_lo .. dist_hi away: half at
    their vertices, edge midpoints and interior points from off their front, half corner_rays at `boxes` (the leaf child boxes that
    lie within the cluster)."""
    h = n // 2
    pick = np.asarray(idx)[rs.randint(0, len(idx), h)]
    v = np.asarray(pos, D)[pick]
    w = rs.dirichlet((1, 1, 1), h)
    w[0::8], w[1::8], w[2::8], w[3::8], w[4::8], w[5::8] = (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (0, 0.5, 0.5), (0.5, 0, 0.5)
    tgt = (v * w[:, :, None]).sum(1)
    nrm = _unit(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    off = _unit(nrm + 0.9 * rs.standard_normal((h, 3)))
    off = np.where(((off * nrm).sum(1) < 0.05)[:, None], nrm, off)
    dist = 2.0 ** rs.uniform(np.log2(dist_lo), np.log2(dist_hi), h)
    first = _aim((tgt + off * dist[:, None]).astype(F), tgt.astype(F))
    return np.concatenate([first, corner_rays(rs, n - h, boxes, dist_lo, dist_hi)])


def condition_number(pos):
    """kappa = |E1| |E2| / |E1 x E2| of triangles (m, 3, 3), float64 (inf for a zero area)."""
    v = np.asarray(pos, D)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    cr = np.cross(e1, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((e1 * e1).sum(1) * (e2 * e2).sum(1)) / np.sqrt((cr * cr).sum(1))


# ---------------------------------------------------------------------------------------------------------------------------------
# acceptance, restated: Triangle::hit and the reference's leaf box as tri_test (csrc/pt_trace.h) evaluates them
# ---------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], -(a[..., 0] * b[..., 2] - a[..., 2] * b[..., 0]),
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def tri_accepts(trees, rays8):
    """(ok (m, n), t (m, n)) for m non-degenerate rays against the n records of trees.tri, in float32 as tri_test forms them: Triangle::hit
    (back-face cull at EPS, 0 <= t <= tmax, u, v) and the reference's slab test on the triangle's reference leaf box."""
    r = np.asarray(rays8, F)
    tri = trees.tri
    org, d = r[:, None, 0:3], r[:, None, 3:6]
    V0, E1, E2 = tri[None, :, 0:3], tri[None, :, 4:7], tri[None, :, 8:11]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        T = org - V0
        Pv, Q = _cross(d, E2), _cross(T, E1)
        det = _dot(Pv, E1)
        t = _dot(Q, E2) * (F(1) / det)
        u = _dot(Pv, T)
        v = _dot(Q, np.broadcast_to(d, T.shape))
        ok = ~(det < EPS) & ~((t < 0) | (t > r[:, None, 7])) & ~((u < 0) | (u > det)) & ~((v < 0) | ((v + u) > det))
        inv, _, _ = ray_setup(r[:, 3:6])
        lb = trees.leafbox[tri[:, 7].view(np.int32)]
        i, j = np.nonzero(ok)
        box_ok, _ = box_test(lb[j, 0:6], r[i, 0:3], inv[i], F(np.inf))
        ok[i, j] = box_ok
    return ok, t.astype(F)


def closest_among(trees, ok, t):
    """(t (m,), prim (m,)) of the closest accepted record per ray, the largest primitive index among equal t (RayCast's tie rule); a
    miss is (0, -1), as pt_trace_rays reports it."""
    tt = np.where(ok, t, F(np.inf))
    best = tt.min(1)
    prim = np.where(ok & (tt == best[:, None]), trees.prim_of[None, :], -1).max(1)
    hit = ok.any(1)
    return np.where(hit, best, F(0)).astype(F), np.where(hit, prim, -1).astype(np.int32)


def walk_result(trees, rays8, which="quad", slack=K_SL):
    """What a walk of the 4-wide tree ("quad", quad_order widened by `slack`) or of the binary tree can return for m rays, as far as the
    chains decide it.  A dict: ok, t (m, n) of tri_accepts; a_lo (m, n), the accepted triangles whose whole chain lets the ray through
    with the cull at the triangle's own t and the smallest cull scale the device can form - the walk is bound to test each of these,
    whatever its order, unless it already holds a closer hit -; a_hi, the same with no cull at all - a triangle outside it is never
    reached -; lo and hi, (t, prim) of the closest hit among each.  The walk's answer is a member of a_hi no farther than lo; where lo
    and hi agree it is that hit."""
    r = np.asarray(rays8, F)
    ok, t = tri_accepts(trees, r)
    i, j = np.nonzero(ok)
    out = {"ok": ok, "t": t}
    for key, cull in (("lo", t[i, j]), ("hi", r[i, 7])):
        if which == "quad":
            acc = quad_chain_accepts(trees, r[i], trees.prim_of[j], cull, slack)
        else:
            acc = binary_chain_accepts(trees, r[i], trees.prim_of[j], cull)
        a = np.zeros_like(ok)
        a[i, j] = acc
        out["a_" + key], out[key] = a, closest_among(trees, a, t)
    return out

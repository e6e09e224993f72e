"""The yardstick of tests/test_query_filters.py (include/pt_api.h, "Query filters"), independent of the code under test: a filtered query
answers over a SUBSET of the set its unfiltered twin is defined over, so the yardsticks that exist (ray_hits_ref.brute, nearest_k_ref
through lists_ref, all in CSR form: offsets, key, prim[, detail]) become the new one by a numpy selection.  And the seeded recipe of
the filters the tests run, built from the reference's own lists."""
import numpy as np

F = np.float32
PRIM_WORDS = np.array([0, 1, 2, 0x80000000, 0x80000001, 0xFFFFFFFF], np.uint32)      # what a primitive's word is drawn from
UNIFORM_MASKS = (0, 1, 0x80000001, 0xFFFFFFFF)
QUERY_WORDS = np.array([0, 1, 2, 3, 0x80000000, 0xFFFFFFFF], np.uint32)               # what a query's word is drawn from
KS = (1, 2, 5, 8, 9, 32)


def owners(off):
    """(total,) the query of every record of a CSR list."""
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def select(H, prim_bits, m, skip, tmin):
    """H' of the header from H = (offsets, key, prim[, detail]): the records with (prim_bits[prim] & m_i) != 0, prim != skip_i and
    not (key < tmin_i), in H's order.  prim_bits: (n_prims,) uint32 or None (every bit set); m: a word or (n,) uint32; skip: (n,) ints or
    None; tmin: (n,) float32 or None."""
    off, key, prim = H[0], H[1], H[2]
    n = len(off) - 1
    own = owners(off)
    words = np.full(len(prim), 0xFFFFFFFF, np.uint32) if prim_bits is None else np.asarray(prim_bits, np.uint32)[prim]
    mask = np.broadcast_to(np.asarray(m, np.uint32), (n,))[own]
    keep = (words & mask) != 0
    if skip is not None:
        keep &= prim != np.asarray(skip, np.int64)[own]
    if tmin is not None:
        with np.errstate(invalid="ignore"):
            keep &= ~(np.asarray(key, F) < np.asarray(tmin, F)[own])
    cnt = np.bincount(own[keep], minlength=n).astype(np.int64)
    off2 = np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt, dtype=np.int64)])
    return (off2,) + tuple(np.ascontiguousarray(x[keep]) for x in H[1:])


def cut(H, k):
    """The K form of a CSR list: (key (n, k), prim (n, k)[, detail (n, k, W)]), the first k records of every query, then the miss record
    (0, -1) and zeros."""
    off, key, prim = H[0], H[1], H[2]
    n = len(off) - 1
    own = owners(off)
    slot = np.arange(len(prim)) - off[own]
    live = slot < k
    ko, po = np.zeros((n, k), F), np.full((n, k), -1, np.int32)
    ko[own[live], slot[live]] = key[live]
    po[own[live], slot[live]] = prim[live]
    out = (ko, po)
    if len(H) > 3:
        d = np.zeros((n, k, H[3].shape[1]), F)
        d[own[live], slot[live]] = H[3][live]
        out += (d,)
    return out


def uncut(key, prim, k):
    """The CSR form of the first two arrays of cut(): every row up to its first miss record."""
    cnt = (prim >= 0).sum(1)
    live = np.arange(prim.shape[1])[None, :] < cnt[:, None]
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(cnt, dtype=np.int64)]), np.ascontiguousarray(key[live]), np.ascontiguousarray(prim[live])


def rows(H, lo, m):
    """The CSR list of the queries lo .. lo + m - 1 alone."""
    off = H[0]
    a, b = off[lo], off[lo + m]
    return (off[lo:lo + m + 1] - a,) + tuple(np.ascontiguousarray(x[a:b]) for x in H[1:])


def same(A, B):
    """Are two lists (CSR or K form) the same bits?"""
    return len(A) == len(B) and all(a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
                                    for a, b in zip(A, B))


class Recipe:
    """The filters of one query set, seeded, built from the reference list H of the set (CSR; for rays the PT_HITS_BOTH_SIDES list, of
    which the front list is a subset).  `filters(rays)` yields (name, prim_bits, m, skip, tmin) — tmin only for rays."""

    def __init__(self, H, n_prims, n_tris, seed, rays):
        rs = np.random.RandomState(seed)
        off, key, prim = H[0], H[1], H[2]
        n = len(off) - 1
        cnt = np.diff(off)
        self.n, self.rays = n, rays
        self.prim_bits = PRIM_WORDS[rs.randint(0, len(PRIM_WORDS), n_prims)]
        self.groups = np.where(np.arange(n_prims) < n_tris, 2, 0x80000001).astype(np.uint32)      # the mesh and "the rest": the spheres
        self.query_bits = QUERY_WORDS[rs.randint(0, len(QUERY_WORDS), n)]
        self.all_set = np.full(n_prims, 0xFFFFFFFF, np.uint32)
        # skip: H's first member, a non-member, none — by turns
        i = np.arange(n)
        first = np.full(n, -1, np.int64)
        first[cnt > 0] = prim[off[:-1][cnt > 0]]
        non = np.empty(n, np.int64)
        for q in range(n):
            mine = set(prim[off[q]:off[q + 1]].tolist())
            p = int(rs.randint(0, n_prims))
            while p in mine and len(mine) < n_prims:
                p = (p + 1) % n_prims
            non[q] = p if p not in mine else n_prims + 7      # a list of the whole scene has no non-member: a number that is no primitive
        self.skip = np.where(i % 3 == 0, first, np.where(i % 3 == 1, non, -1)).astype(np.int32)
        self.skip[(i % 9 == 8)] = n_prims + 3      # and beyond the range: skips none
        # tmin: the t of a member (kept), the next float above it (dropped), 0 — by turns; a ray that holds both roots of a sphere takes
        # its entering root, so that the next float above it lies strictly between the two
        self.tmin = None
        if rays:
            t = np.zeros(n, F)
            for q in range(n):
                if cnt[q] == 0 or q % 4 >= 2:
                    continue
                row = prim[off[q]:off[q + 1]]
                j = cnt[q] // 2
                twice = [p for p in np.unique(row[row >= n_tris]) if (row == p).sum() == 2]
                if twice:
                    j = int(np.nonzero(row == twice[0])[0][0])
                v = key[off[q] + j] + F(0)      # -0 + 0 = +0: no negative tmin
                t[q] = v if q % 4 == 0 else np.nextafter(v, F(np.inf))
            self.tmin = t

    def filters(self):
        out = [(f"prim_bits, bits {m:#x}", self.prim_bits, np.uint32(m), None, None) for m in UNIFORM_MASKS]
        out += [(f"groups, bits {m:#x}", self.groups, np.uint32(m), None, None) for m in (1, 2)]
        out += [("prim_bits, query_bits", self.prim_bits, self.query_bits, None, None),
                ("query_bits alone", None, self.query_bits, None, None),
                ("skip alone", None, np.uint32(0xFFFFFFFF), self.skip, None),
                ("every word set, skip none: the filtered kernels on H itself", self.all_set, np.uint32(0xFFFFFFFF), np.full(self.n, -1, np.int32), None)]
        if self.rays:
            out += [("tmin alone", None, np.uint32(0xFFFFFFFF), None, self.tmin),
                    ("all four fields", self.prim_bits, self.query_bits, self.skip, self.tmin)]
        else:
            out += [("all three fields", self.prim_bits, self.query_bits, self.skip, None)]
        return out

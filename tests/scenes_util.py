"""Seeded input generators shared by the tests and oracle/gen_golden.py (pure numpy)."""
import numpy as np

# float offsets inside one 28-float Vertex record (include/mesh.h:21-37)
V_POS, V_NRM, V_UV, V_TAN, V_BIT, V_EMIT, V_ALB, V_SPEC, V_OPA, V_MET, V_ROU, V_U, V_V = 0, 3, 6, 8, 11, 14, 17, 20, 23, 24, 25, 26, 27


def _norm(v):
    return (v / np.sqrt((v * v).sum(-1, keepdims=True))).astype(np.float32)


def make_prims(a, b, c, albedo=(0.7, 0.7, 0.7), emit=(0, 0, 0), rough=1.0, metal=0.0, opacity=1.0, smooth_normals=None):
    """(n,3) float32 vertex arrays -> (n,84) Primitive records with flat normals and the
    tangent fallback of include/model.h:159-171."""
    a, b, c = (np.asarray(x, np.float32) for x in (a, b, c))
    n = a.shape[0]
    nrm = _norm(np.cross(b - a, c - a).astype(np.float32))
    t1 = np.stack([-nrm[:, 2], np.zeros(n, np.float32), nrm[:, 0]], 1)
    t2 = np.stack([np.zeros(n, np.float32), nrm[:, 2], -nrm[:, 1]], 1)
    use1 = (np.abs(nrm[:, 0]) > np.abs(nrm[:, 1]))[:, None]
    tan = _norm(np.where(use1, t1, t2))
    bit = np.cross(nrm, tan).astype(np.float32)
    out = np.zeros((n, 3, 28), np.float32)
    for k, p in enumerate((a, b, c)):
        out[:, k, V_POS:V_POS + 3] = p
        out[:, k, V_NRM:V_NRM + 3] = nrm if smooth_normals is None else smooth_normals[k]
        out[:, k, V_TAN:V_TAN + 3] = tan
        out[:, k, V_BIT:V_BIT + 3] = bit
        out[:, k, V_EMIT:V_EMIT + 3] = emit
        out[:, k, V_ALB:V_ALB + 3] = albedo
        out[:, k, V_SPEC:V_SPEC + 3] = 0.04
        out[:, k, V_OPA] = opacity
        out[:, k, V_MET] = metal
        out[:, k, V_ROU] = rough
    return out.reshape(n, 84)


def jittered_grid(nx, nz, rs):
    """2*nx*nz triangles on a height field; x/z on a regular lattice so centroids tie a lot
    (exercises the unstable-sort tie order of the BVH build)."""
    xs = np.linspace(-10, 10, nx + 1, dtype=np.float32)
    zs = np.linspace(-10, 10, nz + 1, dtype=np.float32)
    h = rs.uniform(0.0, 1.0, (nx + 1, nz + 1)).astype(np.float32)
    h[::3] = 0.5       # flat rows: exact ties on the y axis as well
    A, B, Cc = [], [], []
    for i in range(nx):
        for j in range(nz):
            p00 = (xs[i], h[i, j], zs[j]); p10 = (xs[i + 1], h[i + 1, j], zs[j])
            p11 = (xs[i + 1], h[i + 1, j + 1], zs[j + 1]); p01 = (xs[i], h[i, j + 1], zs[j + 1])
            A += [p00, p00]; B += [p11, p01]; Cc += [p10, p11]
    prims = make_prims(np.array(A), np.array(B), np.array(Cc))
    prims[0].reshape(3, 28)[:, V_EMIT:V_EMIT + 3] = 5.0     # one emissive triangle so the scene is renderable
    return prims


def random_tris48(m, rs):
    """TRI48 records: V0 V1 V2 N0 N1 N2 T0 T1 T2 B0 B1 B2 | MAT(12).  Smooth, distinct vertex frames."""
    v = rs.uniform(-5, 5, (m, 3, 3)).astype(np.float32)
    v[: m // 8, :, 1] = 0.0                                  # some axis-aligned (flat boxes)
    fr = _norm(rs.standard_normal((m, 9, 3)).astype(np.float32))
    mat = rs.uniform(0, 1, (m, 12)).astype(np.float32)
    return np.concatenate([v.reshape(m, 9), fr.reshape(m, 27), mat], 1).astype(np.float32)


def random_spheres16(s, rs):
    c = rs.uniform(-5, 5, (s, 3)).astype(np.float32)
    r = rs.uniform(0.5, 3, (s, 1)).astype(np.float32)
    mat = rs.uniform(0, 1, (s, 12)).astype(np.float32)
    return np.concatenate([c, r, mat], 1).astype(np.float32)


def random_rays10(r, m, tris48, rs, spheres=None):
    """RAY10 records aimed at their primitive; includes edge/vertex hits, back faces, tiny
    t ranges, un-normalised directions, and rays with zero direction components."""
    idx = rs.randint(0, m, r)
    org = rs.uniform(-12, 12, (r, 3)).astype(np.float32)
    if tris48 is not None:
        v = tris48[idx, :9].reshape(r, 3, 3)
        w = rs.dirichlet((1, 1, 1), r).astype(np.float32)
        w[::16] = (1, 0, 0); w[1::16] = (0.5, 0.5, 0); w[2::16] = (0, 0, 1)      # vertices / edge midpoints
        tgt = (v * w[:, :, None]).sum(1).astype(np.float32)
    else:
        tgt = (spheres[idx, :3] + rs.uniform(-1, 1, (r, 3)) * spheres[idx, 3:4]).astype(np.float32)
    d = (tgt - org).astype(np.float32)
    d[3::16] *= -1                                           # pointing away
    d[4::32, 0] = 0.0                                        # zero components
    d[5::64, 1:] = 0.0
    tmin = np.zeros(r, np.float32)
    tmax = np.full(r, 999999.0, np.float32)
    tmax[6::16] = rs.uniform(0, 10, tmax[6::16].shape)       # ranges that cut the hit off
    tmin[7::16] = rs.uniform(0, 10, tmin[7::16].shape)
    normalise = (rs.uniform(0, 1, r) < 0.7).astype(np.float32)
    scale = rs.uniform(0.2, 3.0, (r, 1)).astype(np.float32)
    d = (d * np.where(normalise[:, None] > 0, 1.0, scale / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6))).astype(np.float32)
    return np.concatenate([idx[:, None].astype(np.float32), org, d, tmin[:, None], tmax[:, None], normalise[:, None]], 1).astype(np.float32)


def scene_rays8(r, rs):
    """RAY8 records for the Cornell-room scenes (room is x,z in [-20,20], y in [0,40])."""
    org = np.stack([rs.uniform(-19, 19, r), rs.uniform(1, 39, r), rs.uniform(-19, 30, r)], 1).astype(np.float32)
    d = _norm(rs.standard_normal((r, 3)).astype(np.float32))
    d[::32] = (0, -1, 0); d[1::32] = (1, 0, 0); d[2::32] = (0, 0, -1)            # axis-aligned (degenerate box test)
    d[3::32, 1] = 0.0                                                             # one zero component, not normalised
    # a share of rays aimed at the mesh in the middle of the room
    aim = np.array([0, 11, 0], np.float32) + rs.uniform(-8, 8, (r, 3)).astype(np.float32)
    k = np.arange(r) % 4 == 0
    d[k] = _norm((aim - org)[k])
    d[3::32, 1] = 0.0
    tmax = np.full(r, 999999.0, np.float32)
    tmax[5::16] = rs.uniform(1, 40, tmax[5::16].shape)
    return np.concatenate([org, d, np.zeros((r, 1), np.float32), tmax[:, None]], 1).astype(np.float32)


def test_spheres():
    """Analytic spheres covering the remaining lobes: rough metal (gltfpbr), delta glass
    (pure_refractive), rough glass (refractive) — cf. srcs/renderer.cpp:125-144."""
    def sph(c, r, albedo, opacity, rough, metal):
        return [*c, r, 0, 0, 0, *albedo, 0.04, 0.04, 0.04, opacity, rough, metal]
    return np.array([
        sph((10, 6, 8), 6.0, (1, 1, 1), 0.0, 0.0, 0.0),          # config-4 glass sphere: pure_refractive
        sph((-11, 5, 9), 5.0, (0.9, 0.9, 1.0), 0.0, 0.05, 1.0),  # rough glass: refractive (renderer.cpp:137-144)
        sph((-9, 30, -8), 6.0, (1, 1, 1), 1.0, 0.2, 1.0),        # rough metal: gltfpbr (renderer.cpp:125-135)
    ], np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# attribute_scene: per-vertex frames and materials, glass and mirror triangles, eight lights, exact ties, slivers, zero areas
# ---------------------------------------------------------------------------------------------------------------------------------
ATTR_RAY_SETS = ("scene", "aimed", "leaving", "axis")
MESH_CLASSES = ("delta_glass", "rough_glass", "v1_opacity", "mirror", "plain")


def _unit64(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _cornell_walls():
    """The five walls of pt_scene_gen(0) (host/scenes.cpp: cornell), without its light: 10 triangles."""
    s = 20.0
    quads = [((-s, 0, s), (s, 0, s), (s, 0, -s), (-s, 0, -s), (.73, .73, .73)),                    # floor
             ((-s, 2 * s, -s), (s, 2 * s, -s), (s, 2 * s, s), (-s, 2 * s, s), (.73, .73, .73)),    # ceiling
             ((-s, 0, -s), (s, 0, -s), (s, 2 * s, -s), (-s, 2 * s, -s), (.73, .73, .73)),          # back
             ((-s, 0, s), (-s, 0, -s), (-s, 2 * s, -s), (-s, 2 * s, s), (.65, .05, .05)),          # left
             ((s, 0, -s), (s, 0, s), (s, 2 * s, s), (s, 2 * s, -s), (.12, .45, .15))]              # right
    out = []
    for a, b, c, d, albedo in quads:
        out.append(make_prims([a, a], [b, c], [c, d], albedo=albedo))
    return np.concatenate(out)


def _standin_positions(n, R=10.0, C=(0.0, 11.0, 0.0)):
    """The triangles of pt_scene_gen(1, n)'s bumpy sphere (host/scenes.cpp: standin), in its order.  Evaluated in float64 and rounded
    once, so that the bits do not depend on which float32 sine a numpy build has (they are within an ulp or two of pt_scene_gen's)."""
    def P(i, j):
        th = 3.14159265 * i / n
        ph = 6.2831853 * j / n
        r = R * (1.0 + 0.08 * np.sin(7.0 * th) * np.cos(5.0 * ph))
        return (C[0] + r * np.sin(th) * np.cos(ph), C[1] + r * np.cos(th), C[2] + r * np.sin(th) * np.sin(ph))
    A, B, Cc = [], [], []
    for i in range(n):
        for j in range(n):
            a, b, c, d = P(i, j), P(i + 1, j), P(i + 1, j + 1), P(i, j + 1)
            if i > 0:
                A.append(a); B.append(d); Cc.append(c)
            if i < n - 1:
                A.append(a); B.append(c); Cc.append(b)
    return tuple(np.array(x, np.float64).astype(np.float32) for x in (A, B, Cc))


def _facing(a, b, c, want):
    """The triangle (a, b, c), wound so that its geometric normal points along `want`."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    return (a, b, c) if np.dot(np.cross(b - a, c - a), want) > 0 else (a, c, b)


def attribute_scene(seed, lat_lon=12):
    """A seeded scene with what the three scenes of pt_scene_gen lack.  Returns ((n, 84) float32 Primitive records, groups): groups maps
    an ingredient to the indices of its primitives in the record array (input order), and "mesh_<class>" to those of a mesh class.

    walls    the five walls of pt_scene_gen(0), flat frames, no light.
    mesh     the stand-in of pt_scene_gen(1, lat_lon).  Per VERTEX, independently: a normal pointing roughly away from the centre
             (noise 0.45, so that rays near grazing see a shading normal facing away), tangent and bitangent built on it, albedo,
             specular, metallic, roughness, opacity, u, v.  On a fifth of the triangles the three normals are twice as long.  Vertex 0's
             material is then set by the triangle's class (MESH_CLASSES; Triangle::hit copies mat0 alone): delta glass (opacity 0,
             roughness 0), rough glass (opacity 0, roughness 0.05 .. 0.5), opaque with opacity 0 on vertex 1 only, mirror (opacity 1,
             roughness < 1e-2), plain (opacity 1, roughness 0.02 .. 1); about a quarter each for the first three.
    lights   eight, one after each eighth of the other primitives behind the walls: seven emissive triangles of areas 50 .. 0.005 and
             seven colours (the floor light faces up, the smallest has 0.1 edges), and one whose SECOND vertex alone is emissive.
    dups     40 exact copies of mesh triangles with another albedo: exact ties in t.
    slivers  30 triangles 10 long and 1e-3 wide, nearly along an axis, above the mesh.
    zero     two zero-area triangles (collinear vertices; two equal vertices), not emissive; their flat normal is NaN."""
    rs = np.random.RandomState(seed)
    walls = _cornell_walls()

    # ---- mesh ----
    a, b, c = _standin_positions(lat_lon)
    m = a.shape[0]
    mesh = make_prims(a, b, c).reshape(m, 3, 28)
    centre = np.array([0.0, 11.0, 0.0])
    for k, p in enumerate((a, b, c)):
        nrm = _unit64(_unit64(p.astype(np.float64) - centre) + 0.45 * rs.standard_normal((m, 3)))
        tan = _unit64(np.cross(nrm, rs.standard_normal((m, 3))))
        mesh[:, k, V_NRM:V_NRM + 3] = nrm
        mesh[:, k, V_TAN:V_TAN + 3] = tan
        mesh[:, k, V_BIT:V_BIT + 3] = np.cross(nrm, tan)
        mesh[:, k, V_UV:V_UV + 2] = rs.uniform(0, 1, (m, 2))
        mesh[:, k, V_ALB:V_ALB + 3] = rs.uniform(0.05, 1.0, (m, 3))
        mesh[:, k, V_SPEC:V_SPEC + 3] = rs.uniform(0.01, 0.2, (m, 3))
        mesh[:, k, V_OPA] = rs.uniform(0, 1, m)
        mesh[:, k, V_MET] = rs.uniform(0, 1, m)
        mesh[:, k, V_ROU] = rs.uniform(0.02, 1.0, m)
        mesh[:, k, V_U] = rs.uniform(0, 1, m)
        mesh[:, k, V_V] = rs.uniform(0, 1, m)
    mesh[::3, 0, V_MET] = 0.0
    mesh[1::3, 0, V_MET] = 1.0
    mesh[::5, 0, V_SPEC:V_SPEC + 3] = 0.04
    long_normals = rs.uniform(0, 1, m) < 0.2
    mesh[long_normals, :, V_NRM:V_NRM + 3] *= np.float32(2)
    u = rs.uniform(0, 1, m)
    cls = np.select([u < 0.25, u < 0.5, u < 0.75, u < 0.85], [0, 1, 2, 3], 4)
    rough_glass = rs.uniform(0.05, 0.5, m).astype(np.float32)
    mirror = rs.uniform(0.0, 0.009, m).astype(np.float32)
    mesh[cls == 0, 0, V_OPA], mesh[cls == 0, 0, V_ROU] = 0.0, 0.0
    mesh[cls == 1, 0, V_OPA], mesh[cls == 1, 0, V_ROU] = 0.0, rough_glass[cls == 1]
    mesh[cls == 2, 0, V_OPA], mesh[cls == 2, 1, V_OPA], mesh[cls == 2, 2, V_OPA] = 1.0, 0.0, 1.0
    mesh[(cls == 2) & (np.arange(m) % 2 == 0), 0, V_ROU] = 1.0
    mesh[cls == 3, 0, V_OPA], mesh[cls == 3, 0, V_ROU] = 1.0, mirror[cls == 3]
    mesh[cls == 4, 0, V_OPA] = 1.0
    mesh = mesh.reshape(m, 84)

    # ---- duplicates ----
    pick = np.sort(rs.choice(m, 40, replace=False))
    dups = mesh[pick].copy().reshape(40, 3, 28)
    dups[:, :, V_ALB:V_ALB + 3] = rs.uniform(0.05, 1.0, (40, 1, 3)).astype(np.float32) * np.float32([0.2, 1.0, 0.2])
    dups = dups.reshape(40, 84)

    # ---- slivers ----
    A, B, Cc = [], [], []
    for i in range(30):
        ax = i % 3
        p0 = np.array([rs.uniform(-17, 7), rs.uniform(23, 35), rs.uniform(-17, 7)])
        e_long = np.zeros(3); e_long[ax] = 10.0
        e_long += rs.uniform(-1e-3, 1e-3, 3)
        side = np.cross(e_long, rs.standard_normal(3))
        side *= 1e-3 / np.sqrt((side * side).sum())
        q = _facing(p0, p0 + e_long, p0 + 0.5 * e_long + side, np.array([0.0, 20.0, 60.0]) - p0)      # towards the reference camera
        A.append(q[0]); B.append(q[1]); Cc.append(q[2])
    slivers = make_prims(np.array(A), np.array(B), np.array(Cc), albedo=(0.9, 0.3, 0.7))

    # ---- zero area ----
    with np.errstate(invalid="ignore", divide="ignore"):
        zero = make_prims(np.float32([[-6, 24, 5], [7, 25, -4]]), np.float32([[-4.5, 24, 5], [7, 25, -4]]), np.float32([[-3, 24, 5], [8, 26, -3]]),
                          albedo=(0.5, 0.5, 0.5))

    # ---- lights ----
    down, up = np.array([0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0])
    spec = [   # vertices, facing, emittance
        (((-5, 39.98, -5), (5, 39.98, -5), (5, 39.98, 5)), down, (15, 15, 15)),                        # area 50
        (((8, 39.98, -15), (8.8, 39.98, -15), (8.8, 39.98, 5)), down, (20, 12, 4)),                    # 8
        (((-19.98, 5, -10), (-19.98, 5, 10), (-19.98, 5.4, 10)), np.array([1.0, 0, 0]), (4, 10, 25)),  # 4, on the left wall
        (((11, 0.02, 10), (14, 0.02, 10), (14, 0.02, 13)), up, (6, 30, 6)),                            # 4.5, on the floor, facing up
        (((6, 26, 4), (6.1, 26, 4), (6, 26, 4.1)), down, (4000, 3000, 2000)),                          # 0.005
        (((-5, 30, -19.98), (5, 30, -19.98), (5, 30.2, -19.98)), np.array([0.0, 0, 1]), (30, 5, 30)),  # 1, on the back wall
        (((-13, 18, 6), (-12, 18.3, 6.8), (-13.2, 19, 6.4)), np.array([1.0, -1.0, 1.0]), (25, 25, 5)),  # about 0.5, tilted
        (((-15, 34, -2), (-5, 34, -2), (-5, 34, -1.4)), down, (0, 0, 0)),                              # 3: only vertex 1 is emissive
    ]
    lights = []
    for verts, want, emit in spec:
        q = _facing(*verts, want)
        lights.append(make_prims(*(np.float32([x]) for x in q), albedo=(0, 0, 0), emit=emit))
    lights = np.concatenate(lights)
    lights[7].reshape(3, 28)[1, V_EMIT:V_EMIT + 3] = (5.0, 5.0, 5.0)

    # ---- input order: walls, then the rest in eight parts with a light behind each ----
    body = np.concatenate([mesh, dups, slivers, zero])
    tag = np.concatenate([np.full(m, 1), np.full(40, 2), np.full(30, 3), np.full(2, 4)])
    parts, tags = [walls], [np.zeros(len(walls), int)]
    for k, idx in enumerate(np.array_split(np.arange(len(body)), 8)):
        parts += [body[idx], lights[k:k + 1]]
        tags += [tag[idx], np.array([5])]
    prims = np.ascontiguousarray(np.concatenate(parts), np.float32)
    tags = np.concatenate(tags)
    groups = {name: np.nonzero(tags == t)[0] for t, name in enumerate(("walls", "mesh", "dups", "slivers", "zero", "lights"))}
    for k, name in enumerate(MESH_CLASSES):
        groups["mesh_" + name] = groups["mesh"][cls == k]
    groups["dup_of"] = groups["mesh"][pick]                  # the mesh triangle each duplicate copies
    groups["dark_light"] = groups["lights"][7:8]             # mat0 emittance 0
    return prims, groups


# ---------------------------------------------------------------------------------------------------------------------------------
# needle_scene: long thin triangles whose boxes all overlap — a shallow tree whose traversal stack runs deep
# ---------------------------------------------------------------------------------------------------------------------------------
NEEDLE_CAMERA_POS = (0.0, 20.0, 40.0)      # make_camera(W, H, pos=NEEDLE_CAMERA_POS): the cube's front face covers the frame
# 8192 needles already overflow the 16 LDS entries of wf_trace's stack for 0.76 of the camera rays, but only 0.013 of their node steps
# are taken at a depth >= 16 (tools/stack_lab.cpp); at 16384 it is 0.029, three times the 0.01 tests/test_needle_scene.py asks of the device
NEEDLE_N = 16384
NEEDLE_SEED = 5


def needle_positions(rs, n, side=30.0, centre=(0.0, 20.0, 0.0), centres=None):
    """(n, 9) float32 vertex positions of n needles, and their (n, 3) float64 centres.  Needle i: centre c uniform in the cube (or
    centres[i]), unit direction d from a normal draw, vertices c - 0.4 side d, c + 0.4 side d and c + 0.002 side t, t a unit vector
    perpendicular to d."""
    if centres is None:
        centres = np.asarray(centre, np.float64) + rs.uniform(-0.5, 0.5, (n, 3)) * side
    d = _unit64(rs.standard_normal((n, 3)))
    t = _unit64(np.cross(d, rs.standard_normal((n, 3))))
    pos = np.stack([centres - 0.4 * side * d, centres + 0.4 * side * d, centres + 0.002 * side * t], 1)
    return pos.reshape(n, 9).astype(np.float32), centres


def needle_scene(seed, n=NEEDLE_N, side=30.0, centre=(0.0, 20.0, 0.0)):
    """n needles (needle_positions) in a cube of side `side` around `centre`, under a square light.  Returns ((n + 2, 84) float32
    Primitive records, (n, 9) float32 needle positions, (n, 3) float64 needle centres); the needles come first, in order.

    Every needle is 0.8 side long and 0.002 side wide, so its box overlaps most others': a ray hits three or four children at every
    level of the 4-wide tree and its traversal stack fills at three entries per level, although the tree is shallow.
    Albedo uniform in [0.2, 0.9] per needle; every eighth needle is a mirror (metallic 1, roughness 0).  The light: two emissive triangles,
    a square of side `side` at y = centre_y + 0.75 side facing down, emittance 4 — shadow rays cross the whole stack of needles."""
    rs = np.random.RandomState(seed)
    pos, centres = needle_positions(rs, n, side, centre)
    v = pos.reshape(n, 3, 3)
    prims = make_prims(v[:, 0], v[:, 1], v[:, 2]).reshape(n, 3, 28)
    prims[:, :, V_ALB:V_ALB + 3] = rs.uniform(0.2, 0.9, (n, 1, 3)).astype(np.float32)
    prims[::8, :, V_MET] = 1.0
    prims[::8, :, V_ROU] = 0.0
    cx, cy, cz = (float(x) for x in centre)
    y, h = cy + 0.75 * side, 0.5 * side
    q = [(cx - h, y, cz - h), (cx + h, y, cz - h), (cx + h, y, cz + h), (cx - h, y, cz + h)]
    down = np.array([0.0, -1.0, 0.0])
    light = [make_prims(*(np.float32([x]) for x in _facing(q[i], q[j], q[k], down)), albedo=(0, 0, 0), emit=(4, 4, 4)) for i, j, k in ((0, 1, 2), (0, 2, 3))]
    return np.ascontiguousarray(np.concatenate([prims.reshape(n, 84)] + light), np.float32), pos, centres


def needle_inner_rays(rs, m, side=30.0, centre=(0.0, 20.0, 0.0)):
    """2 m RAY8 records inside the needle cube: m rays from uniform points in unit normal directions with tmax 999999 (a path's bounce
    rays), then m segments from one uniform point to another, tmax their length (a path's shadow rays)."""
    c = np.asarray(centre, np.float64)
    a, b, o = (c + rs.uniform(-0.5, 0.5, (m, 3)) * side for _ in range(3))
    d = _unit64(rs.standard_normal((m, 3)))
    seg = b - a
    ln = np.sqrt((seg * seg).sum(1, keepdims=True))
    rays = np.zeros((2 * m, 8), np.float32)
    rays[:m, 0:3], rays[:m, 3:6], rays[:m, 7] = o, d, 999999.0
    rays[m:, 0:3], rays[m:, 3:6], rays[m:, 7] = a, seg / ln, ln[:, 0]
    return rays


def pinhole_rays(cam):
    """RAY8 records through the pixel centres of a camera (ptamd.make_camera or oracle_lib.make_camera), row-major, unit directions,
    tmax 999999 — the camera path's rays without their jitter."""
    W, H = cam.W, cam.H
    f, u, r = (np.array(v[:], np.float64) for v in (cam.forward, cam.up, cam.right))
    th = np.tan(0.5 * np.radians(float(cam.fovy_deg)))
    py, px = np.mgrid[0:H, 0:W]
    sx = (2.0 * (px.ravel() + 0.5) / W - 1.0) * th * float(cam.aspect)
    sy = (1.0 - 2.0 * (py.ravel() + 0.5) / H) * th
    d = _unit64(f[None, :] + sx[:, None] * r[None, :] + sy[:, None] * u[None, :])
    rays = np.zeros((W * H, 8), np.float32)
    rays[:, 0:3] = np.array(cam.pos[:], np.float32)
    rays[:, 3:6] = d
    rays[:, 7] = 999999.0
    return rays


REL_RMS_TOL = 1e-4          # north_star tolerance


def check_image(img_g, img_o, what):
    """The project's bar for a GPU frame against the oracle's (BASELINE.json north_star): every value finite, relative RMS within 1e-4
    and at least 0.999 of the pixels bit-identical."""
    rr = rel_rms(img_g, img_o)
    same = (np.ascontiguousarray(img_g, np.float32).view(np.uint32) == np.ascontiguousarray(img_o, np.float32).view(np.uint32)).all(-1)
    print(f"{what}: relRMS {rr:.3e}, bit-identical pixels {same.mean():.6f}")
    assert np.isfinite(img_g).all()
    assert rr <= REL_RMS_TOL, f"{what}: relative RMS {rr:.3e} > {REL_RMS_TOL}"
    assert same.mean() >= 0.999, f"{what}: only {same.mean():.5f} of pixels bit-identical"


def _prim_pos(prims, idx):
    return prims[idx].reshape(-1, 3, 28)[:, :, V_POS:V_POS + 3]


def _aim(org, tgt):
    """RAY8 records from org to tgt: dir = (tgt - org) in float32 times a power of two that brings its components into [-1, 1], so the
    ray passes through tgt as exactly as float32 subtraction allows."""
    org, tgt = np.asarray(org, np.float32), np.asarray(tgt, np.float32)
    d = (tgt - org).astype(np.float32)
    e = np.frexp(np.abs(d).max(1))[1]                        # exact: |d|max * 2^-e is in [0.5, 1)
    d = np.ldexp(d, -e[:, None]).astype(np.float32)
    n = len(org)
    return np.concatenate([org, d, np.zeros((n, 1), np.float32), np.full((n, 1), 999999.0, np.float32)], 1).astype(np.float32)


def attribute_rays(prims, groups, seed, n=2000):
    """The seeded ray sets of attribute_scene, n RAY8 records each, directions with components in [-1, 1]:
    scene    scene_rays8.
    aimed    from outside (off the front of the target triangle, inside the room), aimed in float32 at vertices, edge midpoints and
             interior points of the duplicated triangles, the slivers, the mesh and the walls.
    axis     axis-aligned; the origin shares one or two coordinates with a wall or with a vertex (every face of a leaf box is a vertex
             coordinate).
    `leaving_rays` makes the fourth set from the hit records of `scene` and `aimed` (leaving_parents)."""
    rs = np.random.RandomState(seed)
    out = {"scene": scene_rays8(n, rs)}

    pool = np.concatenate([groups["dups"], groups["dup_of"], groups["slivers"], groups["slivers"], groups["mesh"], groups["walls"]])
    idx = pool[np.arange(n) % len(pool)]
    v = _prim_pos(prims, idx).astype(np.float64)
    w = rs.dirichlet((1, 1, 1), n)
    w[::8] = (1, 0, 0); w[1::8] = (0, 1, 0); w[2::8] = (0, 0, 1); w[3::8] = (0.5, 0.5, 0); w[4::8] = (0, 0.5, 0.5); w[5::8] = (0.5, 0, 0.5)
    tgt = (v * w[:, :, None]).sum(1).astype(np.float32)
    tgt[::8], tgt[1::8], tgt[2::8] = v[::8, 0], v[1::8, 1], v[2::8, 2]       # the vertices themselves, bit for bit
    nrm = _unit64(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    off = _unit64(nrm + 0.6 * rs.standard_normal((n, 3)))
    off = np.where(((off * nrm).sum(1) < 0.2)[:, None], nrm, off)
    org = tgt + off * rs.uniform(4, 14, (n, 1))
    org = np.clip(org, [-19.5, 0.5, -19.5], [19.5, 39.5, 19.5]).astype(np.float32)
    out["aimed"] = _aim(org, tgt)

    verts = prims.reshape(-1, 3, 28)[:, :, V_POS:V_POS + 3].reshape(-1, 3)
    verts = verts[np.isfinite(verts).all(1)]
    pv = verts[rs.randint(0, len(verts), n)]
    qv = verts[rs.randint(0, len(verts), n)]
    ax = rs.randint(0, 3, n)
    sign = np.where(rs.uniform(0, 1, n) < 0.5, -1.0, 1.0).astype(np.float32)
    org = np.stack([rs.uniform(-19, 19, n), rs.uniform(1, 39, n), rs.uniform(-19, 19, n)], 1).astype(np.float32)
    kind = np.arange(n) % 4
    o1, o2 = (ax + 1) % 3, (ax + 2) % 3
    r = np.arange(n)
    org[r, o1] = np.where(kind != 3, pv[r, o1], org[r, o1])              # one coordinate of a vertex ...
    org[r, o2] = np.where(kind == 1, qv[r, o2], org[r, o2])              # ... a second one of another vertex ...
    org[r, o2] = np.where(kind == 2, pv[r, o2], org[r, o2])              # ... or the same vertex: the ray runs through it
    wall = np.float32([[-20, 20], [0, 40], [-20, 20]])
    wsel = kind == 3                                                      # on a wall's plane: along it, or starting on it
    along = rs.uniform(0, 1, n) < 0.5
    org[r, o1] = np.where(wsel & along, wall[o1, rs.randint(0, 2, n)], org[r, o1])
    start_on = wsel & ~along
    near = np.where(sign > 0, wall[ax, 0], wall[ax, 1])                  # the wall behind the ray: start on its plane, or half a unit off it
    org[r, ax] = np.where(start_on, near, near + sign * np.float32(0.5))
    d = np.zeros((n, 3), np.float32)
    d[r, ax] = sign
    out["axis"] = np.concatenate([org, d, np.zeros((n, 1), np.float32), np.full((n, 1), 999999.0, np.float32)], 1).astype(np.float32)
    return out


def leaving_parents(rays, hits_scene, hits_aimed):
    """The rays `leaving_rays` starts from, and their HIT records: the first half of the `scene` set and the first half of `aimed`."""
    h = len(rays["scene"]) // 2
    return np.concatenate([rays["scene"][:h], rays["aimed"][:h]]), np.concatenate([hits_scene[:h], hits_aimed[:h]])


def leaving_rays(rays, hits, seed):
    """Rays leaving the hit points of `rays` (their HIT records: `hits`) along +-n * 1e-4, n the record's normal: even rows start just
    under the surface and go in, odd rows start just above it and go out; where the parent ray missed, the row repeats the parent."""
    rs = np.random.RandomState(seed)
    n = len(rays)
    out = np.ascontiguousarray(rays, np.float32).copy()
    hit = hits[:, 0] > 0
    side = np.where(np.arange(n) % 2 == 0, np.float32(-1), np.float32(1))[:, None]
    nrm = hits[:, 8:11]
    org = (hits[:, 5:8] + side * nrm * np.float32(1e-4)).astype(np.float32)
    d = (side * nrm + np.float32(0.7) * rs.standard_normal((n, 3)).astype(np.float32)).astype(np.float32)
    d = (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(np.float32)
    ok = hit & np.isfinite(org).all(1) & np.isfinite(d).all(1)
    out[ok, 0:3], out[ok, 3:6], out[ok, 7] = org[ok], d[ok], 999999.0
    return out


def bxdf_inputs(n, rs, lobe):
    """Random BxDF table rows (columns 0..23 of pt_dbg_bxdf / o_bxdf's in28) and their seed words (columns 24..25)."""
    nrm = rs.standard_normal((n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    t = np.cross(nrm, rs.standard_normal((n, 3))); t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    front = (rs.uniform(0, 1, (n, 1)) < 0.5).astype(np.float64)
    albedo = rs.uniform(0, 1, (n, 3)); spec = rs.uniform(0, 0.2, (n, 3))
    spec[::5] = 0.04; spec[1::11] = 0.0
    rough = rs.uniform(0.02, 1.0, (n, 1)); rough[::7] = 1.0
    if lobe in (1, 3):
        rough[:] = 0.0
    metal = rs.uniform(0, 1, (n, 1)); metal[::3] = 0.0; metal[1::3] = 1.0
    wo = rs.standard_normal((n, 3)); wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    wi = rs.standard_normal((n, 3)); wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    if lobe < 2:   # opaque lobes are evaluated with wo on the normal's side, as the integrator does
        s = np.sign((wo * nrm).sum(1, keepdims=True)); wo *= np.where(s == 0, 1, s)
    seeds = rs.randint(0, 2 ** 31, (n, 2)).astype(np.uint32).view(np.float32)
    return np.concatenate([nrm, t, b, front, albedo, spec, rough, metal, wo, wi], 1).astype(np.float32), seeds


def rel_rms(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def load_ref_bxdf(golden_dir, lobe):
    """tests/golden/ref_bxdf.npz for one lobe -> (in28, rows in contract mode, rows in glibc mode, number of random rows).  The random
    rows come first and are regenerated from the recorded seed (their sha256 is in the fixture); the hand-built edge block follows."""
    import hashlib
    import os
    g = np.load(os.path.join(golden_dir, "ref_bxdf.npz"))
    n = int(g["n_random"])
    a, seeds = bxdf_inputs(n, np.random.RandomState(int(g["seed"]) + lobe), lobe)
    rnd = np.concatenate([a, seeds, np.zeros((n, 2), np.float32)], 1)
    assert hashlib.sha256(np.ascontiguousarray(rnd).tobytes()).hexdigest() == str(g[f"random_sha256_{lobe}"]), "random BxDF rows drifted"
    in28 = np.concatenate([rnd, g[f"edge_in28_{lobe}"]])
    contract = g[f"contract_{lobe}"]
    glibc = contract.copy()
    glibc[g[f"glibc_idx_{lobe}"]] = g[f"glibc_rows_{lobe}"]
    assert in28.shape[0] == contract.shape[0]
    return in28, contract, glibc, n


ATTR_NEE_ROWS = 2048


def attr_tri_to_input(prims, tris88):
    """For every TRI record of a BVH built from `prims`, the index of its primitive in the input order.  Keyed by the nine vertex floats
    and vertex 0's albedo (a duplicate differs from its original in the albedo alone)."""
    key = {}
    for i, p in enumerate(np.ascontiguousarray(prims, np.float32)):
        key[np.concatenate([p[0:3], p[28:31], p[56:59], p[V_ALB:V_ALB + 3]]).tobytes()] = i
    assert len(key) == len(prims)
    return np.array([key[np.concatenate([t[0:9], t[54:57]]).tobytes()] for t in np.ascontiguousarray(tris88, np.float32)])


def attr_nee_rows(hits, seed, n=ATTR_NEE_ROWS):
    """o_nee's in5 from HIT records: the hit points of the first 70 % of the rows that hit, then hit points pushed 1e-3 under their surface."""
    rs = np.random.RandomState(seed)
    h = hits[(hits[:, 0] > 0) & np.isfinite(hits[:, 5:11]).all(1)]
    assert len(h) >= n
    k = (7 * n) // 10
    pts = np.concatenate([h[:k, 5:8], (h[k:n, 5:8] - np.float32(1e-3) * h[k:n, 8:11]).astype(np.float32)]).astype(np.float32)
    seeds = rs.randint(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([pts, seeds.view(np.float32)], 1)


def load_ref_attr(golden_dir):
    """tests/golden/ref_attr.npz -> (fixture, prims, groups, {set: rays8}, NEE rows in5).  Scene and rays are regenerated from the recorded seed and
    held against their recorded sha256; the `leaving` set and the NEE rows are derived from the fixture's own HIT records."""
    import hashlib
    import os
    g = np.load(os.path.join(golden_dir, "ref_attr.npz"))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()      # noqa: E731
    seed, n = int(g["seed"]), int(g["n_rays"])
    prims, groups = attribute_scene(seed, int(g["lat_lon"]))
    assert sha(prims) == str(g["prims_sha256"]), "attribute_scene drifted"
    rays = attribute_rays(prims, groups, seed + 1, n)
    rays["leaving"] = leaving_rays(*leaving_parents(rays, g["hits_scene"], g["hits_aimed"]), seed + 2)
    for name in ATTR_RAY_SETS:
        assert sha(rays[name]) == str(g[f"rays_sha256_{name}"]), f"ray set {name} drifted"
    in5 = attr_nee_rows(np.concatenate([g["hits_scene"], g["hits_aimed"]]), seed + 3)
    assert sha(in5) == str(g["nee_in5_sha256"]), "NEE rows drifted"
    return g, prims, groups, rays, in5

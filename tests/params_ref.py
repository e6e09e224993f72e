"""Scenes, rows and parameter sets of tests/test_params.py — test infrastructure only.

The integrator reads five caller-set numbers from PtParams: rr_floor, rr_bounce, max_refract, max_bounce, spp_per_pass.  A row of ROWS
is one render at a corner of their ranges: a scene, the fields it overrides, the neighbour row whose frame must differ from its own
and the least share of pixels in which it must (a condition on the INPUT, checked on the CPU oracle alone: a row whose frame did not
depend on its parameter would let a library with the parameter hard-wired pass).  Scenes, cameras and frame sizes are constants here;
every expectation is computed by the oracle at test time."""
import collections
import functools

import numpy as np

import oracle_lib as O
import ptamd
from scenes_util import V_SPEC, _facing, make_prims
from scenes_util import test_spheres as make_test_spheres

NAN, INF = float("nan"), float("inf")
DEFAULT_CAMERA_POS = (0.0, 20.0, 60.0)
MIRROR_CAMERA_POS = (0.0, 20.0, 8.0)
PANE_SPECULAR = 0.0004      # make_prims' 0.04 reflects 1 - 0.96^250 of the paths away before sheet 250; with 0 the oracle's frame is NaN behind the stack

# scene -> frame size, passes and samples of its rows, camera position (default rotation and field of view)
Frame = collections.namedtuple("Frame", "W H passes spp cam_pos")
FRAMES = {
    "standin": Frame(96, 40, 2, 4, DEFAULT_CAMERA_POS),      # the frame of test_gpu_parity.test_short_paths_and_single_samples
    "panes12": Frame(32, 24, 1, 4, DEFAULT_CAMERA_POS),
    "panes256": Frame(32, 24, 1, 4, DEFAULT_CAMERA_POS),
    "mirror": Frame(16, 16, 1, 2, MIRROR_CAMERA_POS),
    "limit": Frame(8, 8, 1, 1, DEFAULT_CAMERA_POS),          # one tile, one pass: 64 streams; spp is the row's
}
LIMIT_WINDOW = (3, 3, 5, 5)      # the oracle renders this window of the 8 x 8 frame only: 65535 samples of all 64 pixels take it 7 s


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes: ((n, 84) float32 Primitive records, (s, 16) float32 spheres or None)
# ---------------------------------------------------------------------------------------------------------------------------------
def standin_spheres():
    """pt_scene_gen(1, 16) with the three analytic spheres of scenes_util.test_spheres: every lobe, refraction chains in the frame."""
    return ptamd.gen_scene(1, 16), make_test_spheres()


def _quad(p0, p1, p2, p3, want, **mat):
    """Two triangles (p0 p1 p2), (p0 p2 p3) whose geometric normals point along `want`."""
    tris = [_facing(p0, p1, p2, want), _facing(p0, p2, p3, want)]
    a, b, c = (np.float32([t[k] for t in tris]) for k in range(3))
    return make_prims(a, b, c, **mat)


def pane_stack(n, specular=PANE_SPECULAR):
    """The Cornell room pt_scene_gen(0) with n sheets of delta glass between the default camera and the room: sheet k = 1 .. n spans
    x in [-8, 8], y in [12, 28] at z = 30 - 0.05 k, normal +z (towards the camera), albedo 1, roughness 0, opacity 0, the given
    specular on all three vertices.  A path that goes straight through is refracted once per sheet, and `refractCnt++ > max_refract`
    ends it at sheet max_refract + 2: the room behind the stack is seen through it only while n <= max_refract + 1."""
    sheets = []
    for k in range(1, n + 1):
        z = 30.0 - 0.05 * k
        q = _quad((-8, 12, z), (8, 12, z), (8, 28, z), (-8, 28, z), np.array([0.0, 0.0, 1.0]), albedo=(1, 1, 1), rough=0.0, opacity=0.0)
        q.reshape(-1, 3, 28)[:, :, V_SPEC:V_SPEC + 3] = specular
        sheets.append(q)
    return np.ascontiguousarray(np.concatenate([ptamd.gen_scene(0)] + sheets), np.float32), None


def mirror_box():
    """A closed cube of side 20 around (0, 20, 0), 12 inward-facing triangles of albedo 1, roughness 0, metallic 1 (the reflective lobe:
    the path weight stays 1, so no path ends before max_bounce unless it finds the light), and under its ceiling a 4 x 4 light at
    y = 29.98 facing down, emittance 20, albedo 0.  A diffuse box would not do: its frames stop changing near 100 bounces."""
    c, h = np.array([0.0, 20.0, 0.0]), 10.0
    faces = []
    for ax in range(3):
        u, v = np.eye(3)[(ax + 1) % 3] * h, np.eye(3)[(ax + 2) % 3] * h
        for sgn in (-1.0, 1.0):
            o = c + sgn * h * np.eye(3)[ax]
            faces.append(_quad(o - u - v, o + u - v, o + u + v, o - u + v, c - o, albedo=(1, 1, 1), rough=0.0, metal=1.0))
    y = 29.98
    light = _quad((-2, y, -2), (2, y, -2), (2, y, 2), (-2, y, 2), np.array([0.0, -1.0, 0.0]), albedo=(0, 0, 0), emit=(20, 20, 20))
    return np.ascontiguousarray(np.concatenate(faces + [light]), np.float32), None


SCENES = {
    "standin": standin_spheres,
    "panes12": lambda: pane_stack(12),
    "panes256": lambda: pane_stack(256),
    "mirror": mirror_box,
    "limit": standin_spheres,
    # the two stacks that do NOT work, kept as a test of why the specular is what it is
    "panes256_spec04": lambda: pane_stack(256, 0.04),
    "panes256_spec0": lambda: pane_stack(256, 0.0),
}
FRAMES["panes256_spec04"] = FRAMES["panes256_spec0"] = FRAMES["panes256"]


@functools.lru_cache(maxsize=None)
def built(scene):
    """(nodes, tris, spheres) of a scene, built once per process and shared by the oracle and the GPU scene."""
    prims, sph = SCENES[scene]()
    nodes, tris, _ = ptamd.build_bvh(prims)
    return nodes, tris, sph


@functools.lru_cache(maxsize=None)
def oracle_scene(scene):
    nodes, tris, sph = built(scene)
    return O.Scene(nodes.tobytes(), tris, sph)


# ---------------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------------
# id | scene | PtParams fields the row overrides | the row it must differ from | least share of pixels that differ | on the GPU too |
# every value finite | the window the oracle renders (None: the frame)
Row = collections.namedtuple("Row", "id scene over neighbour min_share gpu finite window", defaults=(True, True, None))

# Least shares: about a quarter of what the oracle gave when the rows were chosen.  Where that was not measured
# beforehand the bound is the quarter of the smallest measured share among the row's kin: max_refract 0, 1, 3 on the stand-in scene
# gave 0.268, 0.230, 0.180 -> 0.04; 8 against 250 panes gave 0.104 -> 0.025; the combined row and the roulette in the mirror box change
# the random sequence of every path that reaches the roulette, like the rr rows -> their 0.08 and the box's 0.2.
ROWS = (
    Row("default", "standin", {}, None, 0.0, gpu=False),
    Row("rr_floor_0", "standin", dict(rr_floor=0.0), "default", 0.08),
    Row("rr_floor_0.05", "standin", dict(rr_floor=0.05), "default", 0.08),
    Row("rr_floor_1", "standin", dict(rr_floor=1.0), "default", 0.08),
    Row("rr_floor_2", "standin", dict(rr_floor=2.0), "default", 0.08),
    Row("rr_floor_neg1", "standin", dict(rr_floor=-1.0), "default", 0.08),
    Row("rr_floor_nan", "standin", dict(rr_floor=NAN), "default", 0.08),
    Row("rr_floor_inf", "standin", dict(rr_floor=INF), "default", 0.08),
    Row("rr_bounce_neg5", "standin", dict(rr_bounce=-5), "default", 0.08),
    Row("rr_bounce_0", "standin", dict(rr_bounce=0), "default", 0.08, gpu=False),
    Row("rr_bounce_7", "standin", dict(rr_bounce=7), "default", 0.08),
    Row("rr_bounce_8", "standin", dict(rr_bounce=8), "default", 0.08),
    Row("rr_bounce_1000", "standin", dict(rr_bounce=1000), "default", 0.08),
    Row("max_refract_0", "standin", dict(max_refract=0), "default", 0.04),
    Row("max_refract_1", "standin", dict(max_refract=1), "default", 0.04),
    Row("max_refract_3", "standin", dict(max_refract=3), "default", 0.04),
    Row("max_refract_9", "standin", dict(max_refract=9), "default", 0.02),
    Row("max_refract_250", "standin", dict(max_refract=250), "default", 0.02),
    Row("combined", "standin", dict(rr_floor=0.05, rr_bounce=1, max_refract=1, max_bounce=5), "default", 0.08),
    Row("panes12_refract_10", "panes12", dict(max_refract=10), "panes12_refract_11", 0.05),
    Row("panes12_refract_11", "panes12", dict(max_refract=11), "panes12_refract_10", 0.05),
    Row("panes256_refract_8", "panes256", dict(max_refract=8), "panes256_refract_250", 0.025),
    Row("panes256_refract_249", "panes256", dict(max_refract=249), "panes256_refract_250", 0.015),
    Row("panes256_refract_250", "panes256", dict(max_refract=250), "panes256_refract_249", 0.015),
    Row("mirror_bounce_254", "mirror", dict(max_bounce=254, rr_bounce=1000), "mirror_bounce_255", 0.2),
    Row("mirror_bounce_255", "mirror", dict(max_bounce=255, rr_bounce=1000), "mirror_bounce_254", 0.2),
    Row("mirror_bounce_255_rr3", "mirror", dict(max_bounce=255, rr_bounce=3), "mirror_bounce_255", 0.2),
    # the sample limit: all four pixels of the window differ from the row with one sample fewer.  65535 samples are the oracle's alone:
    # one wave takes an MI355X 26 s in the one-kernel mode and 12 s in wf_drain; 32769 still sets bit 31 of the
    # packed stream state
    Row("limit_spp_65535", "limit", dict(spp_per_pass=65535, max_bounce=1), "limit_spp_65534", 1.0, gpu=False, window=LIMIT_WINDOW),
    Row("limit_spp_65534", "limit", dict(spp_per_pass=65534, max_bounce=1), "limit_spp_65535", 1.0, gpu=False, window=LIMIT_WINDOW),
    Row("limit_spp_32769", "limit", dict(spp_per_pass=32769, max_bounce=1), "limit_spp_32768", 1.0, window=LIMIT_WINDOW),
    Row("limit_spp_32768", "limit", dict(spp_per_pass=32768, max_bounce=1), "limit_spp_32769", 1.0, gpu=False, window=LIMIT_WINDOW),
    # lost discrimination, documented: see test_params.test_a_pane_stack_needs_its_small_specular
    Row("spec04_refract_249", "panes256_spec04", dict(max_refract=249), None, 0.0, gpu=False),
    Row("spec04_refract_250", "panes256_spec04", dict(max_refract=250), None, 0.0, gpu=False),
    Row("spec0_refract_250", "panes256_spec0", dict(max_refract=250), None, 0.0, gpu=False, finite=False),
)
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS) and all(r.neighbour is None or r.neighbour in BY_ID for r in ROWS)
FRAME_ROWS = tuple(r for r in ROWS if r.gpu and r.scene != "limit")      # every integrator and schedule renders these
LIMIT_ROWS = tuple(r for r in ROWS if r.gpu and r.scene == "limit")


def row_fields(row):
    """The path parameters of a row, by their PtParams names: the scene's passes and samples, the defaults both libraries share
    (pt_params_default, oracle_lib.make_params), then the row's overrides."""
    f = FRAMES[row.scene]
    fields = dict(passes=f.passes, spp_per_pass=f.spp, max_bounce=8, rr_bounce=3, rr_floor=0.5, max_refract=8, first_pass=0)
    assert set(row.over) <= set(fields), row.id
    fields.update(row.over)
    return fields


def params_pair(row, window=None, **more):
    """The same parameter set for the oracle and for the library: (oracle_lib.OParams, ptamd.PtParams).  `more` overrides fields of
    both (first_pass); `window` is the oracle's pixel window (its seeds stay those of the full frame)."""
    f = FRAMES[row.scene]
    fields = {**row_fields(row), **more}
    op = O.make_params(f.W, f.H, fields["passes"], fields["spp_per_pass"], max_bounce=fields["max_bounce"], rr_bounce=fields["rr_bounce"],
                       rr_floor=fields["rr_floor"], max_refract=fields["max_refract"], first_pass=fields["first_pass"], window=window)
    return op, ptamd.default_params(**fields)


def cameras(row, pos=None, rot=(0.0, 90.0, 0.0), fovy_deg=45.0):
    """(oracle camera, library camera) of a row's frame; another position, rotation or field of view for the batch of views."""
    f = FRAMES[row.scene]
    pos = f.cam_pos if pos is None else pos
    return O.make_camera(f.W, f.H, pos=pos, rot=rot, fovy_deg=fovy_deg), ptamd.make_camera(f.W, f.H, pos=pos, rot_deg=rot, fovy_deg=fovy_deg)


def oracle_frame(row, nthreads=16, **cam):
    """The oracle's frame of a row in contract libm mode: (H, W, 3) float32, read-only; pixels outside the row's window are 0."""
    old = O.set_libm(1)
    try:
        op, _ = params_pair(row, window=row.window)
        img, _ = oracle_scene(row.scene).render(cameras(row, **cam)[0], op, nthreads)
    finally:
        O.set_libm(old)
    img.setflags(write=False)
    return img


def crop(img, window):
    x0, y0, x1, y1 = window
    return img[y0:y1, x0:x1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_pixels(a, b):
    """Per pixel: all three floats have the same bits, NaN taken equal to NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all(-1)


def share_that_differs(a, b):
    return float(1.0 - same_pixels(a, b).mean())

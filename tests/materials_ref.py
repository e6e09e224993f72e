"""The yardstick of tests/test_materials.py, independent of the code under test: what pt_scene_update_materials means for the
`tris` array a fresh upload would be given (include/pt_api.h: "Materials and lights of an uploaded scene"), the light test and the
emittance test of pt_scene_create in numpy float32 (every operation rounds once), and the seeded material sets the tests apply.

Composes with dynamic_ref.restate_tris / refit_nodes for moved geometry: restate_tris(apply_materials(tris, mat), pos)."""
import numpy as np

from dynamic_ref import T_AREA, T_MAT0, T_NORMAL

F = np.float32
MAT_FLOATS = 12                                      # emittance albedo specular opacity roughness metallic
T_MATS = (T_MAT0, T_MAT0 + 12, T_MAT0 + 24)          # mat0 mat1 mat2 of a PtTriangle
THRESHOLD = F(0.0001)
FORCED = (0, 63, 64, 255, 256, 1023, 1024)           # triangles set (b) always lights, where they exist: the edges of waves and blocks


def materials(tris):
    """(n, 12) float32: mat0 of every triangle (what the device shades with)."""
    return np.ascontiguousarray(tris[:, T_MAT0:T_MAT0 + 12], F).copy()


def apply_materials(tris, mat12):
    """tris with mat0 = mat1 = mat2 = mat12[i]; nothing else changes."""
    t = np.ascontiguousarray(tris, F).copy()
    m = np.ascontiguousarray(mat12, F).reshape(-1, MAT_FLOATS)
    assert m.shape[0] == t.shape[0]
    for o in T_MATS:
        t[:, o:o + 12] = m
    return t


def is_light(mat12):
    """pack_surfaces' test on one material per row: sqrtf((ex*ex + ey*ey) + ez*ez) > 0.0001f.  NaN makes no light."""
    e = np.ascontiguousarray(mat12, F)[:, 0:3]
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        assert ln.dtype == F
        return ln > THRESHOLD


def lights_of(tris):
    """The triangles pt_scene_create makes lights: any of the three vertex materials passes the test."""
    return is_light(tris[:, T_MATS[0]:]) | is_light(tris[:, T_MATS[1]:]) | is_light(tris[:, T_MATS[2]:])


def emittance_ok(mat12, spheres=None):
    """emittance_ok of pt_scene_create: every emittance finite, >= 0 and <= 1e8 (triangles: mat0; spheres: floats 4..6)."""
    e = [np.ascontiguousarray(mat12, F)[:, 0:3].ravel()]
    if spheres is not None and len(spheres):
        e.append(np.ascontiguousarray(spheres, F).reshape(-1, 16)[:, 4:7].ravel())
    e = np.concatenate(e)
    with np.errstate(invalid="ignore"):
        return bool((np.isfinite(e) & (e >= 0) & (e <= F(1e8))).all())


def light_records(tris):
    """(n_lights, 16) float32 as the `lights` device array: V0 V1 V2 normal area 0 0 0 of the lights in ascending triangle index."""
    t = tris[lights_of(tris)]
    out = np.zeros((len(t), 16), F)
    out[:, 0:9], out[:, 9:12], out[:, 12] = t[:, 0:9], t[:, T_NORMAL:T_NORMAL + 3], t[:, T_AREA]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the material sets.  Every emittance component is 0 or at least 0.5, i.e. far from the 1e-4 threshold, except for the one pair of
# set (b) that straddles it.
# ---------------------------------------------------------------------------------------------------------------------------------
def set_a(tris, seed):
    """Seeded random albedo, specular, opacity, roughness and metallic; the emittances kept."""
    rs = np.random.RandomState(seed)
    n = len(tris)
    m = materials(tris)
    m[:, 3:6] = rs.uniform(0.05, 1.0, (n, 3))
    m[:, 6:9] = rs.uniform(0.0, 0.2, (n, 3))
    m[:, 9] = rs.choice([1.0, 1.0, 1.0, 0.0], n)             # a quarter of the triangles refract
    m[:, 10] = rs.choice([0.0, 0.005, 0.05, 0.3, 1.0], n) * rs.uniform(0.5, 1.0, n)
    m[:, 11] = rs.choice([0.0, 1.0, 0.5], n)
    return m


def straddle_pair(tris, seed):
    """The two triangles of set (b) that get (1.1e-4, 0, 0) — a light — and (0.9e-4, 0, 0) — none; None for a scene too small."""
    on = _emitting(tris, seed)
    free = np.flatnonzero(~on)
    return (int(free[0]), int(free[1])) if len(free) >= 2 else None


def _emitting(tris, seed):
    n = len(tris)
    on = np.random.RandomState(seed).uniform(size=n) < 0.3
    on &= ~lights_of(tris)                                  # the uploaded lights go off (unless FORCED names one)
    for i in FORCED + (n - 1,):
        if i < n:
            on[i] = True
    return on


def set_b(tris, seed):
    """The uploaded lights off; a seeded 30 % of all triangles emit, and FORCED and n - 1 where they exist; the straddling pair."""
    rs = np.random.RandomState(seed + 1)
    n = len(tris)
    m = materials(tris)
    on = _emitting(tris, seed)
    m[:, 0:3] = np.where(on[:, None], rs.uniform(0.5, 6.0, (n, 3)), 0.0)
    pair = straddle_pair(tris, seed)
    if pair is not None:
        m[pair[0], 0:3] = (1.1e-4, 0.0, 0.0)
        m[pair[1], 0:3] = (0.9e-4, 0.0, 0.0)
    return m


def set_c(tris):
    """Exactly one light: the last triangle."""
    m = materials(tris)
    m[:, 0:3] = 0.0
    m[-1, 0:3] = (12.0, 11.0, 9.0)
    return m


def set_d(tris):
    """No light."""
    m = materials(tris)
    m[:, 0:3] = 0.0
    return m


def set_e(tris):
    """The uploaded materials (mat0) again."""
    return materials(tris)


def material_sets(tris, seed):
    """(name, mat12) of the sets (a) .. (e), in the order the tests apply them."""
    return [("a", set_a(tris, seed)), ("b", set_b(tris, seed)), ("c", set_c(tris)), ("d", set_d(tris)), ("e", set_e(tris))]

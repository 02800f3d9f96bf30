"""The case matrix of the seeded flood's tests (test_dsm_watershed_cpu.py, test_dsm_watershed_gpu.py) and their closed-form
scenes.  A case is a tuple whose first entry names its builder; case(c) gives the arguments of dsm_watershed_oracle.chain:
z, marker, domain, polarity, offset.  numpy only."""
import numpy as np

import dsm_hydro_oracle as ho
import dsm_label_oracle as lo

NODATA = np.float32(-999.0)
BIG = 2 ** 24
OFFSETS = (0, 1, -1, BIG, -BIG)


def seeds_of(z, kind, seed=0):
    """A marker grid for z: nodata where no seed is.  none, corner, centre, every, random (1 % of the cells, at least one)."""
    gh, gw = z.shape
    m = np.full((gh, gw), NODATA, np.float32)
    if kind == "corner":
        m[0, 0] = z[0, 0]
    elif kind == "centre":
        m[gh // 2, gw // 2] = z[gh // 2, gw // 2]
    elif kind == "every":
        m = z.copy()
    elif kind == "random":
        pick = np.random.default_rng(seed + 7).random((gh, gw)) < 0.01
        pick[(gh * 2) // 3, gw // 3] = True
        m[pick] = z[pick]
    else:
        assert kind == "none"
    return m


def _hills(gh, gw, seed, voids=0.0, levels=None):
    z = ho.hills(gh, gw, seed, voids, levels)
    if gh * gw > 4:                                           # the seeds of "corner" and "centre" stand on heights
        for r, c in ((0, 0), (gh // 2, gw // 2)):
            if not ho.valid(z)[r, c]:
                z[r, c] = np.float32(120.0)
    return z


def grid_case(gh, gw, i):
    """Random hills of the given size; polarity, offset and the kind of seeds cycle with i."""
    z = _hills(gh, gw, 10 + i, 0.05 if gh * gw > 100 else 0.0, 9 if i % 2 else None)
    kind = ("random", "every", "corner", "centre")[i % 4]
    return dict(z=z, marker=seeds_of(z, kind, i), domain=None, polarity=(1, -1)[i % 2], offset=OFFSETS[i % 5])


def town_case(voids, polarity, offset, kind):
    z = _hills(257, 301, 3, voids, 24)
    return dict(z=z, marker=seeds_of(z, kind, 3), domain=None, polarity=polarity, offset=offset)


def marker_case(polarity, offset):
    """Markers above, below and equal to the surface, and NaN, +-Inf, nodata and one beyond 32768 m among them."""
    gh, gw = 45, 52
    z = _hills(gh, gw, 21, 0.05, 16)
    rng = np.random.default_rng(5)
    m = (z + rng.choice(np.array([-3.0, -1.0 / 256.0, 0.0, 1.0 / 256.0, 2.5], np.float32), (gh, gw))).astype(np.float32)
    odd = rng.random((gh, gw))
    m[odd < 0.5] = NODATA
    m[(odd >= 0.5) & (odd < 0.55)] = np.nan
    m[(odd >= 0.55) & (odd < 0.58)] = np.inf
    m[(odd >= 0.58) & (odd < 0.61)] = -np.inf
    m[(odd >= 0.61) & (odd < 0.63)] = np.float32(40000.0)
    return dict(z=z, marker=m, domain=None, polarity=polarity, offset=offset)


def domain_case():
    """A domain that cuts the one component of a void-free grid in two; the seeds all lie in the left half, so the right half
    stays at +infinity."""
    gh, gw = 40, 70
    z = _hills(gh, gw, 31, 0.0, 12)
    domain = np.ones((gh, gw), np.uint8)
    domain[:, 33:35] = 0
    m = seeds_of(z, "random", 31)
    m[:, 33:] = NODATA
    return dict(z=z, marker=m, domain=domain, polarity=-1, offset=0)


def spiral_case():
    """A one-cell corridor between walls, spiralling inwards on 97 x 97, level throughout and seeded at its outer end: the flood
    crosses tile borders again and again, and d runs into the thousands."""
    path = lo.spiral(97, 97) != 0
    z = np.where(path, np.float32(50.0), NODATA).astype(np.float32)
    m = np.full_like(z, NODATA)
    m[0, 0] = 50.0
    return dict(z=z, marker=m, domain=None, polarity=1, offset=0)


def constant_case(kind):
    z = np.full((40, 45), 12.25, np.float32)
    return dict(z=z, marker=seeds_of(z, kind), domain=None, polarity=-1, offset=0)


def quantum_case(polarity):
    """Heights on quantisation halves (ties to even), both zeros, NaN, +-Inf, nodata, +-32768 and one ulp beyond; the markers
    likewise."""
    gh, gw = 33, 40
    rng = np.random.default_rng(77)

    def draw():
        a = ((rng.integers(0, 200, (gh, gw)) + 0.5 * rng.integers(0, 2, (gh, gw))) / 256.0).astype(np.float32)
        a[rng.random((gh, gw)) < 0.3] *= -1
        return a
    z, m = draw(), draw()
    z[2, 3], z[2, 4], z[5, 5], z[5, 9], z[9, 9], z[20, 20] = 0.0, -0.0, np.nan, np.inf, -np.inf, NODATA
    z[12, 30], z[12, 31] = 32768.0, np.nextafter(np.float32(32768.0), np.float32(np.inf))
    z[25, 7], z[25, 8] = -32768.0, np.nextafter(np.float32(-32768.0), np.float32(-np.inf))
    m[rng.random((gh, gw)) < 0.7] = NODATA
    m[12, 30], m[25, 7], m[2, 3], m[2, 4] = -32768.0, 32768.0, -0.0, 0.0
    m[3, 3], m[3, 4] = np.nextafter(np.float32(32768.0), np.float32(np.inf)), np.nextafter(np.float32(-32768.0), np.float32(-np.inf))
    return dict(z=z, marker=m, domain=None, polarity=polarity, offset=0)


SIDES = (31, 32, 33, 63, 64, 65)
GRID_CASES = [("grid", 1, 1, 1), ("grid", 1, 70, 2), ("grid", 67, 1, 3), ("grid", 2, 2, 4)] + \
             [("grid", a, b, 5 + i) for i, (a, b) in enumerate(zip(SIDES, SIDES[::-1]))]
TOWN_CASES = [("town", 0.0, -1, 0, "random"), ("town", 0.05, 1, 1, "random"), ("town", 0.3, -1, -1, "random"),
              ("town", 0.05, -1, BIG, "every"), ("town", 0.0, 1, -BIG, "every")]
SEED_CASES = [("town", 0.05, 1, 0, "none"), ("town", 0.0, -1, 0, "corner"), ("town", 0.0, 1, 0, "centre"), ("town", 0.3, 1, 0, "every")]
OTHER_CASES = [("marker", 1, 0), ("marker", -1, 0), ("marker", -1, 700), ("marker", 1, -1), ("domain",), ("spiral",), ("constant", "corner"),
               ("constant", "none"), ("quantum", 1), ("quantum", -1)]
SMALL_CASES = GRID_CASES + OTHER_CASES
ALL_CASES = SMALL_CASES + TOWN_CASES + SEED_CASES
_BUILDERS = {"grid": grid_case, "town": town_case, "marker": marker_case, "domain": domain_case, "spiral": spiral_case,
             "constant": constant_case, "quantum": quantum_case}


def case(c):
    return _BUILDERS[c[0]](*c[1:])


def case_id(c):
    return "-".join(str(v) for v in c)


# ---- closed forms --------------------------------------------------------------------------------------------------------------
CONES = dict(gh=41, gw=56, row=20, col_a=12, col_b=30, h_a=20.0, h_b=14.0, saddle_col=24, saddle=8.0, wall_col=50, wall=30.0)


def two_cones():
    """Two pyramids (Chebyshev cones, 1 m a cell) of 20 m and 14 m on one row over a floor of 0 m, the saddle between them at 8 m
    in column 24, and a wall of 30 m along the east edge: the prominences are 20 m (A, over the floor to the wall) and 6 m (B,
    over the saddle to A); the wall, the highest ground, is a peak at every h.  -> z float32."""
    s = CONES
    r, c = np.mgrid[0:s["gh"], 0:s["gw"]]
    a = s["h_a"] - np.maximum(abs(r - s["row"]), abs(c - s["col_a"]))
    b = s["h_b"] - np.maximum(abs(r - s["row"]), abs(c - s["col_b"]))
    z = np.maximum(0.0, np.maximum(a, b))
    z[:, s["wall_col"]:] = s["wall"]
    return z.astype(np.float32)


TERRACE = dict(gh=40, gw=60, col0=8, row0=6, depth=10, period=8, houses=4, eave=6.0, rise=0.75, tree_row=28, tree_cols=(14, 21), tree_tops=(8.0, 7.5))


def terrace():
    """An nDSM on a 5 m grid: four gabled houses that share walls (ridges along the columns, 9 m, the valleys between them at the
    eaves' 6 m, one column each) and two tree domes of 8 m and 7.5 m, 7 cells apart, whose pass lies at 5.25 m, 2.25 m under the
    lower top; 0 m of ground round them.  extract_objects sees two objects; split at h = 2 m there are six.  -> above float32."""
    s = TERRACE
    z = np.zeros((s["gh"], s["gw"]), np.float32)
    o = np.arange(s["period"] * s["houses"] + 1) % s["period"]
    roof = (s["eave"] + s["rise"] * np.minimum(o, s["period"] - o)).astype(np.float32)
    z[s["row0"]:s["row0"] + s["depth"], s["col0"]:s["col0"] + len(roof)] = roof[None, :]
    r, c = np.mgrid[0:s["gh"], 0:s["gw"]]
    for dome in tree_domes():
        z = np.maximum(z, dome.astype(np.float32))
    return z.astype(np.float32)


def tree_domes():
    s = TERRACE
    r, c = np.mgrid[0:s["gh"], 0:s["gw"]]
    return [top - 0.25 * ((r - s["tree_row"]) ** 2 + (c - col) ** 2) for col, top in zip(s["tree_cols"], s["tree_tops"])]


def terrace_expected():
    """(labels int32 of the six segments in raster order, loose bool): where loose is set (the valley columns, one cell wide) a
    cell may belong to either neighbour; everywhere else the segment is fixed."""
    s = TERRACE
    z = terrace()
    want = np.zeros(z.shape, np.int32)
    loose = np.zeros(z.shape, bool)
    rows = slice(s["row0"], s["row0"] + s["depth"])
    for k in range(s["houses"]):
        c = s["col0"] + k * s["period"]
        want[rows, c:c + s["period"] + 1] = k + 1
        loose[rows, c] = k > 0
    r = np.mgrid[0:z.shape[0], 0:z.shape[1]][0]
    d = tree_domes()                                         # a cell belongs to the dome that is the higher one there
    tree = (z > 2.5) & (r > s["row0"] + s["depth"] + 2)
    want[tree & (d[0] > d[1])] = 5
    want[tree & (d[1] > d[0])] = 6
    assert not (tree & (d[0] == d[1])).any()
    return want, loose

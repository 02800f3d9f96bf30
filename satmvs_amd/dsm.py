"""DSM production: per-view height maps (image space, RPC cameras) fused into one height grid in map coordinates.

    grid = grid_for(heights, rpcs, proj, res=5.0)              # extent of every valid point, cell centres on multiples of res
    dsm = heights_to_dsm(heights, rpcs, proj, grid)            # (gh, gw) float32, nodata where no point fell
    write_dsm("out.tif", dsm, grid)                            # float32 TIFF + world file (.tfw)

and its clean-up, before the DSM is rendered or carries an orthophoto (both out of place, reading the input grid only):

    dsm = despike(dsm, radius=2, thresh=10.0, min_valid=3)     # cells far from their window's median, or nearly alone -> nodata
    dsm = fill_voids(dsm, max_steps=32, min_hits=3)            # voids seen from >= 3 of 8 directions <- inverse-distance mean

and the split into terrain and what stands on it (progressive morphological filter, then the same void filling):

    dtm = extract_dtm(dsm, grid, max_radius=16)                # bare ground: buildings and trees removed and interpolated over
    above = ndsm(dsm, dtm)                                     # heights above ground, >= 0; nodata where either has none
    opened = morph(dsm, radius=8, op="open")                   # the building block: erode / dilate / open / close

and the objects that stand on the ground (connected components in scipy.ndimage.label's numbering, exact statistics):

    labels, stats = extract_objects(above, grid)               # > 2.5 m, >= 50 m^2: area, bbox, centroid, mean, max, volume
    labels, n = label(above > 10.0, connectivity=4)            # the building block; label_stats(), sieve_labels()
    voids, n_voids = label(~(np.isfinite(dsm) & (dsm != -999.0)))   # the void regions fill_voids could not reach

and the planar faces of those objects, roof by roof (facets in exact integers, a least-squares plane per facet):

    labels, n = facets(dsm, grid, tol=0.25, slope_tol=0.1)     # cells whose 3 x 3 windows are planar, linked pairwise; the rims grown
    table = facet_planes(labels, n, dsm, grid)                 # plane, slope_deg, aspect_deg, area_m2, surface_m2, rms_m per facet
    roofs, table = extract_roofs(dsm, above, grid)             # extract_objects -> facets -> facet_planes -> sieve; into outlines()

and the figures of an object that survive outliers, exact order statistics per label of any zone map:

    per = label_quantiles(labels, n, above, q=(0.5, 0.9))      # n_valid, lo, hi (input values, their own bits), value float64
    spread = label_nmad(labels, n, above)                      # median, mad, nmad = 1.4826 mad per label
    score = dsm_metrics_robust(dsm, gt)                        # n, median, nmad, le68, le90, le95; compare_dsms_robust() round a shift

and what the neighbourhood of every cell looks like at any radius, from exact summed-area tables built once per DSM:

    tables = focal_tables(dsm)                                 # one int64 scan per DSM: count, sum and sum of squares in units of 2^-8 m
    position = tpi(dsm, grid, radius=250.0, tables=tables)     # height minus the mean over a disc; dev() divides by the disc's std
    rough = roughness(dsm, focal_window("disc", 50.0, grid=grid), tables=tables)   # any window: "box", "disc", "annulus"
    overview, coarse, count = aggregate(dsm, grid, factor=8)   # block means on the coarser DSMGrid; focal_fraction() for masks
    landform = slope_position(dtm, grid, radius=250.0)         # valley, lower / middle / upper slope, flat, ridge

and what no sum can say about it, exact selections within a window of up to +-32 cells:

    smooth = focal_median(dsm, focal_window("disc", 50.0, grid=grid))   # edge-preserving; focal_quantiles() for any level
    clean = despike_robust(dsm, focal_window("box", 7))        # |z - median| > max(3 nmad, 0.5 m) of focal_nmad() -> nodata
    share = elevation_percentile(dsm, focal_window("disc", 100.0, grid=grid))   # the cell's rank in its window, 0 .. 1

and their outlines as vector data, one polygon with holes per object, and polygons put back on the grid:

    rings = outlines(labels, len(stats["area"]), grid)         # rings of lattice corners: exterior counter-clockwise, holes clockwise
    write_geojson("objects.geojson", rings, grid, stats)       # a FeatureCollection with the statistics as properties
    again = burn_rings(rings["vertices"], rings["offset"], rings["label"], labels.shape)   # == labels; for label_stats over footprints

and the terrain as vector data, contour lines at many levels in one call:

    lines = contours(dtm, interval=2.5, grid=grid)             # ordered float64 vertex lists: open chains and closed rings
    write_contours("contours.geojson", lines, grid)            # a FeatureCollection of LineStrings: level_m, closed, length_m

and water over the terrain: depressions filled, D8 directions, accumulation, catchments (what every DTM package offers):

    filled, depth, flat = fill_depressions(dtm, return_depth=True)   # the lowest surface without pits; depth = filled - dtm, exact
    direction = flow_direction(dtm, grid)                      # uint8: 0 outlet, k + 1 towards E, SE, S, SW, W, NW, N, NE, 255 invalid
    acc = flow_accumulation(direction, grid=grid)              # upstream area [m^2] (cells without a grid; int32 weights)
    basin, n = basins(direction, pour_points=[(row, col)])     # catchments of the pour points (of every outlet without them)
    rivers = streams(acc, 1e4)                                 # the cells that drain 1 ha or more
    labels, stats, depth = depressions(dtm, grid)              # >= 0.5 m deep, >= 50 m^2, as objects: into outlines(), write_geojson()
    links = stream_links(direction, rivers, grid=grid)         # Strahler orders, links with next_link, polylines, length_m
    write_streams("streams.geojson", links, grid, proj)        # or extract_streams(dtm, grid) for the whole chain
    metres = flow_length(direction, grid=grid)                 # every cell's way to its root (step counts without a grid)

and distance over ground that is not uniformly passable: accumulated cost, the source that serves each cell, least-cost paths:

    friction = quantise_friction(1.0 + slope(dtm, grid) / 10.0)      # cost per metre as uint16 in units of 2^-8; 0 = a barrier
    cost, backlink = cost_distance(sources, grid, friction)    # float64 cost metre (+Inf unreachable, NaN barrier); a D8 forest
    cost, backlink = cost_distance(sources, grid, dsm=dtm, vertical=tobler_table())   # walking effort: the slope along each step
    served_by, n = cost_allocation(backlink)                   # = basins(backlink): the source each cell's cheapest trip ends at
    paths = least_cost_paths(backlink, targets, grid)          # the trips of the targets as merged links, into write_streams()

and objects that have merged into one blob split at their saddles: a flood from chosen cells at chosen levels (the seeded flood):

    lower = h_maxima(above, 2.0)                               # every dome cut down to what stands less than 2 m over its saddle
    tops, n, table, dome = peaks(above, 2.0, grid)             # the top plateaus of the domes with a prominence of 2 m or more
    segments = watershed(above, tops, mask=above > 2.5)        # every cell to the peak it is reached from over the highest pass
    labels, n, table = split_objects(above, grid, h=2.0)       # extract_objects -> peaks -> watershed; into outlines(), write_geojson()
    rec = reconstruct(marker, dsm, "dilation")                 # the building block; "erosion"; h_minima(); open_by_reconstruction()

and the surface itself as a triangle mesh with a guaranteed error (adaptive RTIN), for viewers, engines, printing, texturing:

    errors = mesh_errors(dtm, tile=256)                        # once per DSM: the exact error of every hierarchy triangle, saturated
    m = mesh(dtm, grid, tol=0.5, errors=errors)                # vertices, z, triangles, tri_level, xyz: every height within tol of it
    h, dev = mesh_heights(dtm, 0.5, errors=errors, return_dev=True)   # the mesh's height at every cell, and its deviation
    write_ply("dtm.ply", m, grid, colors=ortho_u8)             # binary PLY with the orthophoto's colours; write_obj() with vt

and the comparison with another DSM (a ground truth, a LiDAR DSM, an earlier epoch), after removing the offset between them:

    reg = coregister(dsm, grid, gt, gt_grid)                   # the shift with the least spread of dsm - gt: de, dn, dz, std, grid
    on_gt = regrid(dsm, reg["grid"], gt_grid, dz=-reg["dz"])   # onto the other grid, bilinear or nearest
    scores = compare_dsms(dsm, grid, gt, gt_grid)              # {"shift", "before", "after"}: dsm_metrics around the registration
    diff, labels, stats = changes(new, new_grid, old, old_grid)   # rises and falls above 2.5 m and 50 m^2 as objects

and several DSMs (one per stereo triplet, strip, block or epoch) put together into one, feathered so that no seam shows:

    reg = coregister(tile, g, ref, ref_grid)                   # the tile's offset against what is there already
    whole = mosaic([ref, tile - reg["dz"]], [ref_grid, reg["grid"]], align="bilinear")   # on mosaic_grid(...) of the two
    d = distance(valid, max_dist=64)                           # the building block: cells to the nearest void, exact
    near = buffer_mask(~valid, 2.5)                            # everything within 2.5 cells of a void, for scoring

and the sun over a DSM: cast shadows for a given sun, shaded relief, and exposure over a list of suns:

    shade = cast_shadows(dsm, grid, azimuth=135.0, elevation=30.0)      # uint8: 0 no height, 1 lit, 2 in cast shadow
    relief = hillshade(dsm, grid, azimuth=315.0, elevation=45.0, shadows=True)   # float32 in [0, 1]; slope(), aspect(), gradient()
    exposure = sun_exposure(dsm, grid, suns, weights)          # sum of w cos(incidence) over the suns that reach a cell
    per_roof = label_stats(labels, n, values=exposure)         # "how much sun does this roof get"

and horizon maps, which turn every further sun (or satellite) into a comparison per cell and give the sky-view factor:

    azimuths = horizon_azimuths(16)                            # 0, 22.5, ... degrees clockwise from north
    tan_h = horizon(dsm, grid, azimuths)                       # (16, gh, gw) float32: tangent of the horizon's elevation angle
    svf = sky_view_factor(tan_h)                               # isotropic sky view of a horizontal surface, in [0, 1]
    seen = horizon_lit(tan_h, azimuths, azimuth=100.0, elevation=35.0)   # 0 no height, 1 seen from there, 2 hidden
    exposure = sun_exposure_from_horizon(dsm, grid, tan_h, azimuths, suns, weights)   # sun_exposure without a scan per sun

and viewsheds, what an eye on or above the surface sees (a mast, a roof, a road), with earth curvature and refraction:

    seen = viewshed(dsm, grid, [(row, col)], observer_height=1.6)   # (1, gh, gw) uint8: 0 no height, 1 seen, 2 hidden, 3 out of range
    count = visibility_count(seen)                             # how many observers see each cell
    code = line_of_sight(dsm, grid, a, b)                      # the same rule for pairs of cells; intervisibility(dsm, grid, points)

and the reverse direction, a DSM rendered into one view's image-space heights (e.g. `height/` ground truth for a tile):

    dsm, grid = read_dsm("gt.tif")                             # float32 + its world file
    h = render_heights(dsm, grid, rpc, proj, (H, W), origin=(x0, y0))   # (H, W) float32, NaN where the view sees no DSM
    save_pfm("height.pfm", h)                                  # data_io.save_pfm

and the orthophoto, the views' imagery resampled onto the DSM's grid with occlusion (a true orthophoto):

    ortho, src = orthorectify(images, rpcs, dsm, grid, proj, return_source=True)   # (gh, gw, C) float32, NaN where unseen
    write_ortho("ortho.tif", np.nan_to_num(ortho).clip(0, 255).astype(np.uint8), grid)   # RGB TIFF + world file
    vis = visibility(dsm, grid, rpcs[0], proj, images[0].shape[:2])           # 0 no height, 1 outside, 2 occluded, 3 visible

The hot path is native (include/satmvs.h, smvs_rpc_dsm_bin / smvs_dsm_reduce): one lane per pixel projects (x, y, h) through
the inverse RPC and the Transverse Mercator forward into a cell; the reduce sorts every cell's heights and takes the median /
mean / min / max.  The result is bit-identical from run to run and under any order of the maps.
smvs_rpc_dsm_render marches every pixel's ray down through the bilinear DSM surface and bisects the first crossing.
smvs_dsm_despike takes the median of every cell's window with a sorting network in registers over a tile staged in LDS;
smvs_dsm_fill finds the eight directional hits of every void cell as states carried along columns, diagonals and rows.
smvs_dsm_morph / smvs_dsm_ground take window minima and maxima as row and column passes over order-preserving keys, each a
doubling in LDS whose cost does not grow with the radius but with its logarithm.
smvs_dsm_label is a union-find over cell indices (tiles in LDS, tile borders with integer min atomics, a three-level scan
for the numbering); smvs_dsm_label_stats reduces along rows and columns on chip before its integer atomics.
smvs_dsm_outline_count / _write keep the boundary edges per lattice corner, find every ring's start and every edge's rank by
one pointer doubling over the predecessor permutation, and order rings and vertices by scans; smvs_dsm_burn toggles labels
along vertical edges with integer XOR atomics and takes a running XOR along the rows.
smvs_dsm_contour_count / _write number the crossings (level, lattice edge) by a scan over the edges of the levels that cross
each, link every crossing to its successor in the square it enters, rank open chains and rings by the same pointer doubling,
and write float64 vertices; all levels of a call are in flight at once.
smvs_dsm_flood_begin / _rounds / _read fill depressions as a monotone relaxation of 64-bit keys (filled height, steps within a
flat) over tiles of 32 x 32 cells in LDS, rounds in batches with one read of the device per batch; smvs_dsm_flow_dir is one
lane per cell; smvs_dsm_flow_accumulate ranks an Euler tour of the flow forest by one pointer doubling with int64 suffix sums
and smvs_dsm_flow_basins numbers the roots by a scan: launches follow log(cells), not the longest river.
smvs_dsm_stream_order / _write rank an Euler tour of the forest induced on the stream cells, raise the Strahler order by one
per round through a scan of junction marks at their tour positions, and find every cell's link head by an in-place pointer
doubling; smvs_dsm_flow_length is one doubling over the forest with the three step counts as sums.
smvs_dsm_cost_begin / _rounds / _read are the flood's relaxation with another step rule: uint64 accumulated costs over the same
tiles, the eight integer step costs of a lane's cells in registers, the back-links read off the final keys one lane per cell.
smvs_dsm_seed_begin / _rounds / _read are the flood's relaxation with other ends: a valid cell with a valid marker is a seed at
level s = max(g, polarity q(marker) + offset), K = max((g, 0), min(S, min over the valid neighbours of K + 1)) with +infinity + 1 =
+infinity, invalid and off-grid neighbours are walls, all valid cells are open (another seed may undercut a seed), and the
back-links (0 at a seed with K = S, else the neighbour with the least key, ties to the lowest k) are a D8 forest for basins().
smvs_dsm_mesh_errors is one lane per lattice vertex over all levels of the bisection hierarchy, the deviation from each
triangle's plane raised into its split vertex's word by 64-bit integer max atomics (a wave an 8 x 8 block, its lanes combined per
split vertex first), then one gather pass per level; smvs_dsm_mesh_count / _write flag the emitted triangles per slot of the
output order and place them by scans; smvs_dsm_mesh_heights walks every vertex down its root triangle by the active flags.
smvs_dsm_facet_label is smvs_dsm_label's union-find with another adjacency: the 3 x 3 integer gradients of all cells once into the
workspace, tiles of q, Gx, Gy in LDS, a pair united where its link holds; smvs_dsm_facet_planes reduces int64 moments about
an integer centre along a wave's rows and columns before its atomics, and fits the plane in float64 in a fixed order.
smvs_dsm_label_select is a radix descent over the 32 bits of the order-preserving keys for up to 8 ranks per label at once: a
counting pass per bit (a ballot per rank where a wave lies inside a zone, runs of lanes with one label elsewhere, the waves of a
workgroup combined in LDS before the integer atomics) and one lane per (label, rank) that fixes the bit and lowers the rank.
smvs_dsm_focal_build writes the inclusive 2-D prefix tables of the count, of d = q - centre and of d^2 modulo 2^64: a range pass
(the only atomics, integer), a column pass cut into bands of 16 rows with an exact carry (band totals from the floats, a scan down
the bands, then the prefixes), and a row pass in place, a workgroup per row in segments of 1024 entries with the carry in registers;
smvs_dsm_focal_query is one lane per output cell over a window's rectangle records, four corner reads per table and record, the
variance from an exact 128-bit integer.
smvs_dsm_focal_select stages a 32 x 32 tile and its window's reach as keys in LDS, the window's row runs in the kernel arguments;
every lane then runs a radix descent over its own window, counting from LDS; smvs_dsm_focal_count is one counting pass of the same.
smvs_dsm_shift_stats pairs every cell with its partner under every shift of a square, tiles of both grids in LDS and the
shifts' integer sums in registers; smvs_dsm_regrid is one lane per destination cell.
smvs_dsm_dist is an exact squared Euclidean distance transform in two line passes (rows since the last background cell
carried along columns, then a lower envelope searched outwards along rows in LDS); smvs_dsm_mosaic is one lane per
destination cell over a table of up to 64 layers, float64 sums in the list's order.
smvs_dsm_stack_select / _fuse are one lane per destination cell over the same table, the lane's valid keys kept sorted by
insertion in its own column of LDS: every level is one read, the MAD a merge outwards from the median along that column.
smvs_dsm_shadow is an exclusive running maximum of z - tan(elevation) (distance towards the sun) along sheared lines of
the grid, a lane per line, cut into bands with an exact carry, the east-west directions between tile transposes through LDS;
smvs_dsm_gradient is Horn's 3 x 3 gradient, one lane per cell.
smvs_dsm_horizon walks the same sheared lines with the upper convex hull of the cells passed so far as a stack of links in
memory, slopes compared by exact int64 cross-multiplication, a lane per (direction, line), all directions of a call side by side.
smvs_dsm_viewshed walks one line of sight per (observer, target cell) over heights quantised once per call, the minor
coordinate from an integer error accumulator and every sample compared with the target by an int64 cross-multiplication, a
wave an 8 x 8 block of targets, all observers of a call in one launch.  smvs_dsm_los runs the same device function over a
device list of pairs, reading the floats themselves.
smvs_rpc_ortho projects every cell into a view, marches the ray up through the same surface to test occlusion, and samples
the image bilinearly.
`proj` is a transverse_mercator.TransverseMercator (whu_tlc_projection() for WHU-TLC).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

MODES = {"median": 0, "mean": 1, "min": 2, "max": 3}


@dataclass(frozen=True)
class DSMGrid:
    """A north-up grid: (e0, n0) is the CENTRE of cell (0, 0), the upper-left one; columns run east by xres, rows south by yres."""
    e0: float
    n0: float
    xres: float
    yres: float
    width: int
    height: int

    def grid4(self):
        return np.array([self.e0, self.n0, self.xres, self.yres], dtype=np.float64)

    def cell_of(self, east, north):
        """(col, row) of map points, float64 numpy: the kernel's rule with the same IEEE operations."""
        col = np.floor((np.asarray(east, np.float64) - self.e0) / self.xres + 0.5)
        row = np.floor((self.n0 - np.asarray(north, np.float64)) / self.yres + 0.5)
        return col, row


def _dev():
    if not torch.cuda.is_available():
        raise _lib.SatMVSNativeError("DSM production runs on an MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(x, dtype=None, dev=None):
    """(contiguous device tensor, whether the caller gave numpy).  dev=None: a device tensor stays where it is and anything
    else goes to the current device; dtype=None: the dtype is kept."""
    as_numpy = not isinstance(x, torch.Tensor)
    if dev is None:
        dev = _dev() if as_numpy or not x.is_cuda else x.device
    t = torch.from_numpy(np.ascontiguousarray(x)) if as_numpy else x
    return t.to(device=dev, dtype=dtype).contiguous(), as_numpy


def _back(as_numpy, *results):
    """The way back from _to_device: the results (None stays None) as numpy if the caller gave numpy; a single one bare."""
    out = tuple(t.cpu().numpy() if as_numpy and t is not None else t for t in results)
    return out[0] if len(out) == 1 else out


def _on_grid(a, grid):
    if tuple(a.shape) != (grid.height, grid.width):
        raise ValueError("dsm shape %s differs from the grid's (%d, %d)" % (tuple(a.shape), grid.height, grid.width))
    return a


# A DSM argument follows one of two dtype policies.  Render, orthophoto and production compute new values from the heights,
# so they CONVERT whatever real dtype comes to float32 (_dsm_converted, and _maps for the height maps).  Clean-up and
# morphology copy cells bit for bit, so they REJECT anything that is not float32 already (_dsm_bits): a silent conversion
# would change the bits they promise to keep.
def _dsm_converted(dsm, grid):
    """The DSM of `grid`, numpy taken as float32 (a tensor is converted on its way to the device)."""
    if not isinstance(dsm, torch.Tensor):
        dsm = np.asarray(dsm, dtype=np.float32)
    return _on_grid(dsm, grid)


def _dsm_bits(dsm):
    """A (gh, gw) float32 grid, numpy or tensor, checked before any device work and never converted."""
    if not isinstance(dsm, torch.Tensor):
        dsm = np.asarray(dsm)
    if dsm.ndim != 2:
        raise ValueError("a DSM is (gh, gw), got shape %s" % (tuple(dsm.shape),))
    if dsm.dtype not in (np.float32, torch.float32):
        raise ValueError("a DSM is float32, got %s" % (dsm.dtype,))
    gh, gw = int(dsm.shape[0]), int(dsm.shape[1])
    if gh < 1 or gw < 1 or gh * gw >= 2 ** 31:
        raise ValueError("a DSM has positive sizes and fewer than 2^31 cells, got %d x %d" % (gh, gw))
    return dsm


def _as_list(x, n=None):
    if x is None:
        return [None] * n
    if isinstance(x, (list, tuple)):
        return list(x)
    if (isinstance(x, np.ndarray) or isinstance(x, torch.Tensor)) and x.ndim == 3:
        return [x[i] for i in range(x.shape[0])]
    return [x]


def _rpc_list(rpcs):
    """One RPC, a list of RPCs, or an array of RPCs along its first axis -> a list."""
    if isinstance(rpcs, (list, tuple)):
        return list(rpcs)
    if isinstance(rpcs, (np.ndarray, torch.Tensor)) and rpcs.ndim >= 2:
        return [rpcs[i] for i in range(rpcs.shape[0])]
    return [rpcs]


def _rpc_checked(rpc):
    r = torch.as_tensor(rpc, dtype=torch.float64).reshape(-1) if not isinstance(rpc, torch.Tensor) else rpc.reshape(-1)
    if r.numel() != 170:
        raise ValueError("rpc vectors must hold 170 values, got %d" % r.numel())
    return r


def _valid_range(z, nodata, lower=True):
    """(lowest, highest) valid cell, reduced on the device (the kernel's validity test: float32 cells against (float)nodata).
    lower=False leaves the lowest out (None) for the callers that march upwards only."""
    valid = torch.isfinite(z) & (z != float(np.float32(nodata)))
    h_hi = float(torch.where(valid, z, torch.full_like(z, -math.inf)).amax())
    if not math.isfinite(h_hi):
        raise ValueError("the DSM has no valid cell")
    h_lo = float(torch.where(valid, z, torch.full_like(z, math.inf)).amin()) if lower else None
    return h_lo, h_hi


def _maps(heights, rpcs, masks, dev):
    hs = _as_list(heights)
    rs = _rpc_list(rpcs)
    ms = _as_list(masks, len(hs))
    if len(rs) != len(hs) or len(ms) != len(hs):
        raise ValueError("one RPC (and one mask, if any) per height map: %d maps, %d rpcs, %d masks" % (len(hs), len(rs), len(ms)))
    out = []
    for h, r, m in zip(hs, rs, ms):
        h, _ = _to_device(h, torch.float32, dev)
        if h.ndim != 2:
            raise ValueError("height maps are (H, W), got %s" % (tuple(h.shape),))
        r = _to_device(r, torch.float64, dev)[0].reshape(-1)
        if r.numel() != 170:
            raise ValueError("rpc vectors must hold 170 values")
        if m is not None:
            m = torch.as_tensor(m).to(device=dev)
            if tuple(m.shape) != tuple(h.shape):
                raise ValueError("mask shape %s differs from the height map's %s" % (tuple(m.shape), tuple(h.shape)))
            m = (m != 0).to(torch.uint8).contiguous()
        out.append((h, r, m))
    return out


_call = _lib.launch     # one native call on dev's current stream: tensors as device pointers, numpy arrays as host pointers, None as NULL


def _bin(h, r, m, tm7, grid4, gw, gh, cell, count, east=None, north=None):
    H, W = h.shape
    _call(h.device, "smvs_rpc_dsm_bin", h, m, r, H, W, tm7, grid4, gw, gh, cell, count, east, north)


def project_to_map(heights, rpcs, projection, masks=None):
    """(east, north) float64 device tensors per map; NaN where a pixel is invalid (masked out or a non-finite height)."""
    dev = _dev()
    tm7 = projection.tm7()
    dummy = DSMGrid(0.0, 0.0, 1.0, 1.0, 1, 1).grid4()
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    out = []
    for h, r, m in _maps(heights, rpcs, masks, dev):
        cell = torch.empty(h.shape, dtype=torch.int32, device=dev)
        east = torch.empty(h.shape, dtype=torch.float64, device=dev)
        north = torch.empty_like(east)
        _bin(h, r, m, tm7, dummy, 1, 1, cell, count, east, north)
        out.append((east, north))
    return out


def grid_from_extent(emin, emax, nmin, nmax, res):
    """The grid of resolution `res` whose cells cover [emin, emax] x [nmin, nmax] with cell centres on integer multiples of res
    (so that tiles and runs line up), every extreme point inside by the kernel's cell rule."""
    res = float(res)
    if not res > 0.0 or not all(math.isfinite(v) for v in (emin, emax, nmin, nmax, res)):
        raise ValueError("grid_from_extent needs a finite extent and a positive resolution")
    if emax < emin or nmax < nmin:
        raise ValueError("empty extent")
    e0 = math.floor(emin / res + 0.5) * res
    n0 = math.ceil(nmax / res - 0.5) * res
    g = DSMGrid(e0, n0, res, res, 1, 1)
    c, r = g.cell_of(emin, nmax)
    e0 -= res * max(0.0, -float(c))                          # rounding at a half cell: step one cell outward
    n0 += res * max(0.0, -float(r))
    g = DSMGrid(e0, n0, res, res, 1, 1)
    c, r = g.cell_of(emax, nmin)
    width, height = int(c) + 1, int(r) + 1
    if width * height >= 2 ** 31:
        raise ValueError("grid of %d x %d cells is too large (limit 2^31 cells)" % (width, height))
    return DSMGrid(e0, n0, res, res, width, height)


def grid_for(heights, rpcs, projection, res, masks=None):
    """DSMGrid of resolution `res` [m] over the extent of every valid point of the maps."""
    en = project_to_map(heights, rpcs, projection, masks)
    lo, hi = [math.inf, math.inf], [-math.inf, -math.inf]
    for east, north in en:
        ok = torch.isfinite(east) & torch.isfinite(north)
        if bool(ok.any()):
            e, n = east[ok], north[ok]
            lo = [min(lo[0], float(e.min())), min(lo[1], float(n.min()))]
            hi = [max(hi[0], float(e.max())), max(hi[1], float(n.max()))]
    if not math.isfinite(lo[0]):
        raise ValueError("no valid point in the height maps")
    return grid_from_extent(lo[0], hi[0], lo[1], hi[1], res)


def reduce_cells(cell, height, count, grid, mode="median", nodata=-999.0):
    """The reduce pass alone: cell int32 (n) and height float32 (n) device tensors, count (gw*gh) int32 from the bin pass ->
    (gh, gw) float32 device tensor."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
    dev = cell.device
    n = cell.numel()
    gw, gh = grid.width, grid.height
    nbytes = _lib.load().smvs_dsm_workspace_bytes(n, gw, gh)
    if nbytes == 0:
        raise ValueError("unsupported DSM size: %d points, %d x %d cells (limits: 2^31 points, 2^31 cells)" % (n, gw, gh))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    _call(dev, "smvs_dsm_reduce", cell, height, n, count, gw, gh, MODES[mode], float(nodata), out, ws, nbytes)
    return out


def heights_to_dsm(heights, rpcs, projection, grid, masks=None, mode="median", nodata=-999.0, return_count=False):
    """Fuse height maps (a list of (H, W) maps of any sizes, numpy or device tensors; one 170-vector RPC each; optional masks,
    e.g. filter_depth's final mask) into the DSM of `grid`: every valid pixel goes to the cell its (E, N) falls in, every cell
    takes the `mode` ("median", "mean", "min", "max") of its heights, empty cells get `nodata`.
    -> (gh, gw) float32 (and int32 counts with return_count), numpy if the heights came as numpy, device tensors otherwise."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
    as_numpy = not all(isinstance(h, torch.Tensor) for h in _as_list(heights))
    dev = _dev()
    maps = _maps(heights, rpcs, masks, dev)
    n = sum(h.numel() for h, _, _ in maps)
    if n >= 2 ** 31:
        raise ValueError("too many points for one DSM: %d (limit 2^31)" % n)
    gw, gh = int(grid.width), int(grid.height)
    tm7, grid4 = projection.tm7(), grid.grid4()
    cell = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(gw * gh, dtype=torch.int32, device=dev)
    flat = torch.cat([h.reshape(-1) for h, _, _ in maps]) if len(maps) > 1 else maps[0][0].reshape(-1)
    at = 0
    for h, r, m in maps:                                     # every bin call writes its slice of one cell array
        _bin(h, r, m, tm7, grid4, gw, gh, cell[at:at + h.numel()], count)
        at += h.numel()
    out = reduce_cells(cell, flat, count, grid, mode, nodata)
    out, cnt = _back(as_numpy, out, count.reshape(gh, gw))
    return (out, cnt) if return_count else out


def _int_pair(v, name):
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError("%s must be a pair of integers, got %r" % (name, v)) from None
    if not all(isinstance(t, (int, np.integer)) and not isinstance(t, bool) for t in (a, b)):
        raise ValueError("%s must be a pair of integers, got %r" % (name, v))
    return int(a), int(b)


def _tile(shape, origin):
    """(H, W, x0, y0) of a tile of a view, checked as the native entries check them."""
    H, W = _int_pair(shape, "shape")
    x0, y0 = _int_pair(origin, "origin")
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("shape must be positive with H * W below 2^31, got %r" % (tuple(shape),))
    if x0 < 0 or y0 < 0 or x0 + W > 2 ** 31 - 1 or y0 + H > 2 ** 31 - 1:
        raise ValueError("origin must be non-negative, with x0 + W and y0 + H below 2^31, got %r" % (tuple(origin),))
    return H, W, x0, y0


def render_heights(dsm, grid, rpc, projection, shape, origin=(0, 0), nodata=-999.0, tol=1e-3):
    """Render a DSM into one view: the height each pixel of the view sees (include/satmvs.h
    smvs_rpc_dsm_render for the exact definition).  dsm (grid.height, grid.width) float32 on `grid`, numpy or a device tensor;
    cells equal to `nodata` or non-finite are holes (nodata=float("nan") makes NaN alone mean "no value").  rpc: the view's
    170-vector; shape = (H, W) of the rendered tile, origin = (x0, y0) its upper-left pixel in the view (pixel (i, j) of the tile
    is view column x0 + j, row y0 + i).  Heights are found to within tol [m].
    -> (H, W) float32, NaN where the view sees no DSM; numpy if the DSM came as numpy, a device tensor otherwise."""
    H, W, x0, y0 = _tile(shape, origin)
    tol = float(tol)
    if not (tol > 0.0 and math.isfinite(tol)):
        raise ValueError("tol must be positive and finite, got %r" % tol)
    dsm = _dsm_converted(dsm, grid)
    r = _rpc_checked(rpc)
    dev = _dev()
    z, as_numpy = _to_device(dsm, torch.float32, dev)
    r, _ = _to_device(r, torch.float64, dev)
    h_lo, h_hi = _valid_range(z, nodata)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    _call(dev, "smvs_rpc_dsm_render", z, grid.width, grid.height, grid.grid4(), float(nodata), projection.tm7(), r,
          H, W, x0, y0, h_lo, h_hi, tol, out)
    return _back(as_numpy, out)


# ---- clean-up: speckle removal and void filling ---------------------------------------------------------------------------------
FILL_METHODS = {"idw": 0, "nearest": 1, "min": 2}
MAX_FILL_STEPS = 4096


def _int_checked(v, name, lo, hi):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= v <= hi:
        raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
    return int(v)


def despike(dsm, nodata=-999.0, radius=2, thresh=10.0, min_valid=3, return_removed=False):
    """Remove speckles from a DSM (include/satmvs.h smvs_dsm_despike): a valid cell becomes `nodata` where
    the (2 radius + 1)^2 window around it (clipped at the border, the cell included) holds fewer than min_valid valid cells, or
    where the cell lies more than thresh [m] from the window's median; every other cell is copied bit for bit.  dsm (gh, gw)
    float32, numpy or a device tensor, left untouched; radius 1, 2 or 3; thresh finite and >= 0; 1 <= min_valid <= window size.
    -> the cleaned (gh, gw) float32 (and, with return_removed, a uint8 map of the removed cells); numpy if the DSM came as numpy,
    device tensors otherwise."""
    dsm = _dsm_bits(dsm)
    radius = _int_checked(radius, "radius", 1, 3)
    min_valid = _int_checked(min_valid, "min_valid", 1, (2 * radius + 1) ** 2)
    thresh = float(thresh)
    if not (math.isfinite(thresh) and thresh >= 0.0):
        raise ValueError("thresh must be finite and >= 0, got %r" % thresh)
    z, as_numpy = _to_device(dsm)
    gh, gw = z.shape
    out = torch.empty_like(z)
    removed = torch.empty((gh, gw), dtype=torch.uint8, device=z.device) if return_removed else None
    _call(z.device, "smvs_dsm_despike", z, gw, gh, float(nodata), radius, thresh, min_valid, out, removed)
    out, removed = _back(as_numpy, out, removed)
    return (out, removed) if return_removed else out


def fill_voids(dsm, nodata=-999.0, max_steps=32, min_hits=3, method="idw", return_hits=False):
    """Fill the voids of a DSM (include/satmvs.h smvs_dsm_fill): every invalid cell looks E, NE, N, NW, W,
    SW, S, SE for the first valid cell within max_steps cells; with at least min_hits such hits it takes their inverse-distance
    mean ("idw", float64, weights 1 / distance^2), the nearest of them ("nearest") or the lowest ("min", the ground-side fill for
    occlusion shadows beside buildings); ties keep the earlier direction.  Cells with fewer hits stay as they are, valid cells
    are copied bit for bit, and only the input is read, so filled cells never feed other cells.  dsm (gh, gw) float32, numpy or
    a device tensor, left untouched; 1 <= max_steps <= 4096; 1 <= min_hits <= 8.
    -> the filled (gh, gw) float32 (and, with return_hits, a uint8 map: 255 where the input cell was valid, else its number of
    hits); numpy if the DSM came as numpy, device tensors otherwise."""
    dsm = _dsm_bits(dsm)
    if method not in FILL_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(FILL_METHODS), method))
    max_steps = _int_checked(max_steps, "max_steps", 1, MAX_FILL_STEPS)
    min_hits = _int_checked(min_hits, "min_hits", 1, 8)
    z, as_numpy = _to_device(dsm)
    gh, gw = z.shape
    nbytes = _lib.load().smvs_dsm_fill_workspace_bytes(gw, gh, max_steps)
    if nbytes == 0:
        raise ValueError("unsupported fill: %d x %d cells, max_steps %d" % (gw, gh, max_steps))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    out = torch.empty_like(z)
    hits = torch.empty((gh, gw), dtype=torch.uint8, device=z.device) if return_hits else None
    _call(z.device, "smvs_dsm_fill", z, gw, gh, float(nodata), max_steps, min_hits, FILL_METHODS[method], out, hits, ws, nbytes)
    out, hits = _back(as_numpy, out, hits)
    return (out, hits) if return_hits else out


# ---- ground extraction: morphology, the progressive morphological filter, DTM and nDSM ------------------------------------------
MORPH_OPS = {"erode": 0, "dilate": 1, "open": 2, "close": 3}
MAX_MORPH_RADIUS = 256
MAX_GROUND_LEVELS = 16
GROUND_CLASSES = ("invalid", "ground")                            # 0, 1; 2 + k = removed at level k of the schedule


def _morph_workspace(z, max_radius):
    gh, gw = z.shape
    nbytes = _lib.load().smvs_dsm_morph_workspace_bytes(gw, gh, max_radius)
    if nbytes == 0:
        raise ValueError("unsupported morphology: %d x %d cells, radius %d" % (gw, gh, max_radius))
    return torch.empty(nbytes, dtype=torch.uint8, device=z.device), nbytes


def morph(dsm, radius, op, nodata=-999.0):
    """Grey-scale morphology with a (2 radius + 1)^2 square clipped at the grid border (include/satmvs.h smvs_dsm_morph,
    DESIGN.md section 9): op "erode" = the lowest valid cell of the window, "dilate" = the highest, "open" = the dilation of
    the erosion, "close" = the erosion of the dilation.  Invalid cells are transparent to the windows and are copied bit for
    bit; of two zeros -0.0 is the lower.  dsm (gh, gw) float32, numpy or a device tensor, left untouched; 1 <= radius <= 256.
    -> (gh, gw) float32; numpy if the DSM came as numpy, a device tensor otherwise."""
    dsm = _dsm_bits(dsm)
    radius = _int_checked(radius, "radius", 1, MAX_MORPH_RADIUS)
    if op not in MORPH_OPS:
        raise ValueError("op must be one of %s, got %r" % (sorted(MORPH_OPS), op))
    z, as_numpy = _to_device(dsm)
    gh, gw = z.shape
    ws, nbytes = _morph_workspace(z, radius)
    out = torch.empty_like(z)
    _call(z.device, "smvs_dsm_morph", z, gw, gh, float(nodata), radius, MORPH_OPS[op], out, ws, nbytes)
    return _back(as_numpy, out)


def ground_schedule(cell, max_radius=16, slope=0.3, dh0=1.5, dh_max=6.0):
    """The window radii [cells] and height thresholds [m] of the progressive morphological filter (Zhang et al. 2003): radii
    1, 2, 4, ... below max_radius, then max_radius; w_k = 2 r_k + 1; t_0 = dh0, t_k = min(dh_max, slope (w_k - w_(k-1)) cell +
    dh0), in float64.  cell [m] > 0; slope [m/m], dh0, dh_max [m] finite and >= 0.  -> (list of int, list of float)."""
    max_radius = _int_checked(max_radius, "max_radius", 1, MAX_MORPH_RADIUS)
    cell, slope, dh0, dh_max = float(cell), float(slope), float(dh0), float(dh_max)
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError("cell must be positive and finite, got %r" % cell)
    for name, v in (("slope", slope), ("dh0", dh0), ("dh_max", dh_max)):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
    radii, r = [], 1
    while r < max_radius:
        radii.append(r)
        r *= 2
    radii.append(max_radius)
    thresholds = [dh0]
    for k in range(1, len(radii)):
        thresholds.append(min(dh_max, slope * float((2 * radii[k] + 1) - (2 * radii[k - 1] + 1)) * cell + dh0))
    return radii, thresholds


def _schedule_checked(radii, thresholds):
    radii, thresholds = list(radii), [float(t) for t in thresholds]
    if not 1 <= len(radii) <= MAX_GROUND_LEVELS or len(thresholds) != len(radii):
        raise ValueError("a schedule has 1 .. %d radii and as many thresholds, got %d and %d" % (MAX_GROUND_LEVELS, len(radii), len(thresholds)))
    radii = [_int_checked(r, "radius", 1, MAX_MORPH_RADIUS) for r in radii]
    if any(b <= a for a, b in zip(radii, radii[1:])):
        raise ValueError("radii must be strictly increasing, got %r" % (radii,))
    if not all(math.isfinite(t) and t >= 0.0 for t in thresholds):
        raise ValueError("thresholds must be finite and >= 0, got %r" % (thresholds,))
    return radii, thresholds


def ground_filter(dsm, cell=None, nodata=-999.0, max_radius=16, slope=0.3, dh0=1.5, dh_max=6.0, return_class=False, schedule=None):
    """The progressive morphological ground filter (include/satmvs.h smvs_dsm_ground): the surface is
    opened with the growing windows of ground_schedule(cell, max_radius, slope, dh0, dh_max); a valid cell that level k's
    opening lowers by more than t_k is removed at level k, and the next level works on the opened surface.  cell: the cell
    size [m].  schedule = (radii, thresholds) replaces the schedule of the parameters (cell is not needed then).  The defaults
    are a choice for 5 m grids, not tuned on real data.  dsm (gh, gw) float32, numpy or a device tensor, left
    untouched.
    -> dtm (gh, gw) float32: the input's bits at ground cells, nodata at removed cells, invalid cells copied (and, with
    return_class, cls uint8: 0 invalid input, 1 ground, 2 + k removed at level k); numpy if the DSM came as numpy."""
    dsm = _dsm_bits(dsm)
    if schedule is not None:
        radii, thresholds = _schedule_checked(*schedule)
    else:
        if cell is None:
            raise ValueError("ground_filter needs the cell size [m] (or a schedule)")
        radii, thresholds = ground_schedule(cell, max_radius, slope, dh0, dh_max)
    z, as_numpy = _to_device(dsm)
    gh, gw = z.shape
    ws, nbytes = _morph_workspace(z, radii[-1])
    dtm = torch.empty_like(z)
    cls = torch.empty((gh, gw), dtype=torch.uint8, device=z.device)
    r_arr, t_arr = np.asarray(radii, np.int32), np.asarray(thresholds, np.float64)
    _call(z.device, "smvs_dsm_ground", z, gw, gh, float(nodata), r_arr, t_arr, len(radii), dtm, cls, ws, nbytes)
    dtm, cls = _back(as_numpy, dtm, cls)
    return (dtm, cls) if return_class else dtm


def extract_dtm(dsm, grid, nodata=-999.0, max_radius=16, slope=0.3, dh0=1.5, dh_max=6.0, max_steps=256, min_hits=3, return_class=False):
    """A DTM from a DSM: ground_filter with cell = max(grid.xres, grid.yres), then fill_voids(method="idw") under what was
    removed.  The fill also closes voids the input already had within max_steps cells, which is what a DTM wants; voids out of
    reach stay.  -> dtm (gh, gw) float32 (and the filter's cls with return_class)."""
    _on_grid(dsm, grid)
    max_steps = _int_checked(max_steps, "max_steps", 1, MAX_FILL_STEPS)
    min_hits = _int_checked(min_hits, "min_hits", 1, 8)
    holes, cls = ground_filter(dsm, max(float(grid.xres), float(grid.yres)), nodata, max_radius, slope, dh0, dh_max, return_class=True)
    dtm = fill_voids(holes, nodata=nodata, max_steps=max_steps, min_hits=min_hits, method="idw")
    return (dtm, cls) if return_class else dtm


def ndsm(dsm, dtm, nodata=-999.0, clamp=True):
    """Heights above ground: float32 dsm - dtm where both are valid (one IEEE operation), max(., 0) with clamp, nodata
    elsewhere.  Torch operators on whatever device the inputs are on (numpy in, numpy out)."""
    as_numpy = not isinstance(dsm, torch.Tensor)
    a = torch.as_tensor(np.asarray(dsm) if as_numpy else dsm)
    b = torch.as_tensor(np.asarray(dtm) if not isinstance(dtm, torch.Tensor) else dtm).to(a.device)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.ndim != 2 or a.shape != b.shape:
        raise ValueError("ndsm takes two float32 grids of one shape, got %s %s and %s %s" % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    nd = float(np.float32(nodata))
    both = torch.isfinite(a) & (a != nd) & torch.isfinite(b) & (b != nd)
    d = a - b
    if clamp:
        d = torch.where(d > 0.0, d, torch.zeros_like(d))                  # every zero leaves as +0.0
    return _back(as_numpy, torch.where(both, d, torch.full_like(d, nd)))


# ---- objects: connected components of a mask and their statistics ---------------------------------------------------------------
def _mask_checked(mask):
    if not isinstance(mask, torch.Tensor):
        mask = np.asarray(mask)
        integral = mask.dtype == np.bool_ or np.issubdtype(mask.dtype, np.integer)
    else:
        integral = mask.dtype == torch.bool or not (mask.is_floating_point() or mask.is_complex())
    if mask.ndim != 2:
        raise ValueError("a mask is (gh, gw), got shape %s" % (tuple(mask.shape),))
    if not integral:
        raise ValueError("a mask is bool or an integer type (non-zero = foreground), got %s" % (mask.dtype,))
    gh, gw = int(mask.shape[0]), int(mask.shape[1])
    if gh < 1 or gw < 1 or gh * gw >= 2 ** 31:
        raise ValueError("a mask has positive sizes and fewer than 2^31 cells, got %d x %d" % (gh, gw))
    return mask


def _connectivity_checked(connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
    return int(connectivity)


def _labels_checked(labels):
    if not isinstance(labels, torch.Tensor):
        labels = np.asarray(labels)
    if labels.ndim != 2:
        raise ValueError("labels are (gh, gw), got shape %s" % (tuple(labels.shape),))
    if labels.dtype not in (np.int32, torch.int32):
        raise ValueError("labels are int32, got %s" % (labels.dtype,))
    gh, gw = int(labels.shape[0]), int(labels.shape[1])
    if gh < 1 or gw < 1 or gh * gw >= 2 ** 31:
        raise ValueError("labels have positive sizes and fewer than 2^31 cells, got %d x %d" % (gh, gw))
    return labels


def label(mask, connectivity=8):
    """Connected components of a mask (include/satmvs.h smvs_dsm_label, DESIGN.md section 9, "Objects"): mask (gh, gw), bool or
    any integer dtype, non-zero = foreground (a float mask is rejected: threshold it yourself); connectivity 4 (E, N, W, S) or 8
    (plus the diagonals).  Labels are 1 .. n in raster order of every component's first cell, the numbering of
    scipy.ndimage.label, 0 = background; they depend on the mask alone, bit for bit.
    -> (labels (gh, gw) int32, n int); labels numpy if the mask came as numpy, a device tensor otherwise.  Reading n is the one
    synchronisation."""
    mask = _mask_checked(mask)
    connectivity = _connectivity_checked(connectivity)
    if not isinstance(mask, torch.Tensor):
        mask = np.not_equal(mask, 0).view(np.uint8)          # every integer dtype numpy has, torch's or not
    m, as_numpy = _to_device(mask)
    m = (m != 0).to(torch.uint8).contiguous()
    gh, gw = m.shape
    nbytes = _lib.load().smvs_dsm_label_workspace_bytes(gw, gh)
    if nbytes == 0:
        raise ValueError("unsupported labelling: %d x %d cells" % (gw, gh))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    labels = torch.empty((gh, gw), dtype=torch.int32, device=m.device)
    n_dev = torch.empty(1, dtype=torch.int32, device=m.device)
    _call(m.device, "smvs_dsm_label", m, gw, gh, connectivity, labels, n_dev, ws, nbytes)
    n = int(n_dev.item())
    if n < 0:
        raise _lib.SatMVSNativeError("smvs_dsm_label gave up: a union-find loop reached its bound (n = %d)" % n)
    return _back(as_numpy, labels), n


def label_stats(labels, n, values=None, grid=None, nodata=-999.0):
    """Statistics of the labels 1 .. n of a label map (include/satmvs.h smvs_dsm_label_stats): labels (gh, gw) int32 from
    label(); cells with a label outside 1 .. n count for nothing.  -> dict of arrays of length n, entry k for label k + 1:
      area int32 [cells]; bbox int32 (n, 4) r0, c0, r1, c1 inclusive; rc_sum int64 (n, 2); centroid float64 (n, 2) row, col
      with grid (a DSMGrid of the labels' shape): area_m2, and centroid_en float64 (n, 2) east, north (cell centres)
      with values ((gh, gw) float32, never converted; valid = finite and != nodata): n_valid int32; min, max float32 (by the
        keys' order: -0.0 below +0.0; nodata where n_valid is 0); qsum int64 = the exact sum of the valid values rounded to
        units of 2^-10 m (0.98 mm, far below any DSM's accuracy) and clamped to +-2^21 m; mean float64 = qsum / 1024 / n_valid
        (NaN where n_valid is 0)
      with both: volume float64 = qsum / 1024 * xres * yres [m^3].
    Every sum is an integer sum: equal bits from run to run.  numpy if the labels came as numpy, device tensors otherwise."""
    labels = _labels_checked(labels)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n < 2 ** 31:
        raise ValueError("n must be an integer in 0 .. 2^31 - 1, got %r" % (n,))
    n = int(n)
    if values is not None:
        values = _dsm_bits(values)
        if tuple(values.shape) != tuple(labels.shape):
            raise ValueError("values shape %s differs from the labels' %s" % (tuple(values.shape), tuple(labels.shape)))
    if grid is not None:
        _on_grid(labels, grid)
    lab, as_numpy = _to_device(labels)
    dev = lab.device
    gh, gw = lab.shape
    area = torch.empty(n, dtype=torch.int32, device=dev)
    bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
    rc = torch.empty((n, 2), dtype=torch.int64, device=dev)
    v = nvalid = vmin = vmax = qsum = None
    if values is not None:
        v, _ = _to_device(values, dev=dev)
        nvalid = torch.empty(n, dtype=torch.int32, device=dev)
        vmin = torch.empty(n, dtype=torch.float32, device=dev)
        vmax = torch.empty_like(vmin)
        qsum = torch.empty(n, dtype=torch.int64, device=dev)
    if n:
        _call(dev, "smvs_dsm_label_stats", lab, v, gw, gh, float(nodata), n, area, bbox, rc, nvalid, vmin, vmax, qsum)
    out = {"area": area, "bbox": bbox, "rc_sum": rc, "centroid": rc.double() / area.double()[:, None]}
    if grid is not None:
        out["area_m2"] = area.double() * float(grid.xres) * float(grid.yres)
        out["centroid_en"] = torch.stack([float(grid.e0) + out["centroid"][:, 1] * float(grid.xres),
                                          float(grid.n0) - out["centroid"][:, 0] * float(grid.yres)], dim=1)
    if values is not None:
        some = nvalid > 0
        out.update({"n_valid": nvalid, "min": vmin, "max": vmax, "qsum": qsum,
                    "mean": torch.where(some, qsum.double() / 1024.0 / nvalid.double().clamp(min=1.0), torch.full_like(qsum, float("nan"), dtype=torch.float64))})
        if grid is not None:
            out["volume"] = qsum.double() / 1024.0 * float(grid.xres) * float(grid.yres)
    return {k: _back(as_numpy, t) for k, t in out.items()}


def sieve_labels(labels, area, min_area=1, max_area=None):
    """Drop the components whose area [cells] is outside min_area .. max_area (None: no upper limit): their cells become 0, the
    others are renumbered 1 .. n' in their old order, so still in raster order of their first cells.  labels (gh, gw) int32
    with values 0 .. n, area (n) from label_stats.  Torch operators on whatever device the labels are on.
    -> (labels', n', kept): kept int64 (n') = the old indices (label - 1) of the components that stay."""
    labels = _labels_checked(labels)
    min_area = _int_checked(min_area, "min_area", 0, 2 ** 31 - 1)
    if max_area is not None:
        max_area = _int_checked(max_area, "max_area", min_area, 2 ** 31 - 1)
    as_numpy = not isinstance(labels, torch.Tensor)
    lab = torch.as_tensor(labels)
    a = torch.as_tensor(np.asarray(area) if not isinstance(area, torch.Tensor) else area).to(lab.device)
    if a.ndim != 1 or a.is_floating_point():
        raise ValueError("area is a 1-D integer array, one entry per label, got %s %s" % (a.dtype, tuple(a.shape)))
    keep = a >= min_area
    if max_area is not None:
        keep &= a <= max_area
    new_id = torch.cumsum(keep, 0, dtype=torch.int32) * keep                 # the new label of an old one, 0 if dropped
    lut = torch.cat([torch.zeros(1, dtype=torch.int32, device=lab.device), new_id])
    out = lut[lab.long()]
    kept = torch.nonzero(keep)[:, 0]
    out, kept_out = _back(as_numpy, out, kept)
    return out, int(kept.numel()), kept_out


def extract_objects(above, grid, min_height=2.5, min_area_m2=50.0, connectivity=8, nodata=-999.0):
    """The objects of an nDSM: foreground = the valid cells of `above` ((gh, gw) float32 heights above ground, from ndsm()) with
    above > float32(min_height); label(); label_stats(values=above, grid=grid); sieve_labels() at ceil(min_area_m2 / (xres
    yres)) cells.  The defaults (2.5 m, 50 m^2 = two cells of a 5 m grid) are a choice for 5 m grids, not tuned on
    real data.  -> (labels (gh, gw) int32 with 1 .. n' on the objects that stay, stats: the dict of label_stats restricted to
    them); numpy if `above` came as numpy, device tensors otherwise."""
    above = _on_grid(_dsm_bits(above), grid)
    connectivity = _connectivity_checked(connectivity)
    min_height, min_area_m2 = float(min_height), float(min_area_m2)
    if not math.isfinite(min_height):
        raise ValueError("min_height must be finite, got %r" % min_height)
    if not (math.isfinite(min_area_m2) and min_area_m2 >= 0.0):
        raise ValueError("min_area_m2 must be finite and >= 0, got %r" % min_area_m2)
    min_cells = _int_checked(int(math.ceil(min_area_m2 / (float(grid.xres) * float(grid.yres)))), "min_area_m2 in cells", 0, 2 ** 31 - 1)
    z, as_numpy = _to_device(above)
    fg = torch.isfinite(z) & (z != float(np.float32(nodata))) & (z > float(np.float32(min_height)))
    labels, n = label(fg, connectivity)
    stats = label_stats(labels, n, values=z, grid=grid, nodata=nodata)
    labels, _, kept = sieve_labels(labels, stats["area"], min_cells)
    stats = {k: t[kept] for k, t in stats.items()}
    return _back(as_numpy, labels), {k: _back(as_numpy, t) for k, t in stats.items()}


# ---- facets: planar faces of a DSM (roofs, flat ground) and their planes ------------------------------------------------------------
MAX_FACET_TERM = 2 ** 26                                          # T, Ax, Ay: with it no term of the rule wraps an int32
MAX_FACET_PLANE_SIDE = 32768                                      # facet_planes: gw, gh <= 2^15 and gw gh < 2^24 keep every sum below 2^63
MAX_FACET_PLANE_CELLS = 2 ** 24
FACET_MOMENTS = ("Sx", "Sy", "Sz", "Sxx", "Sxy", "Syy", "Sxz", "Syz")


def _facet_term(v, name):
    if not (math.isfinite(v) and 0.0 <= v <= MAX_FACET_TERM):
        raise ValueError("%s must be in 0 .. 2^26, got %r" % (name, v))
    return int(math.floor(v))


def facet_terms(grid, tol=0.25, slope_tol=0.1):
    """(T, Ax, Ay) of the facet rule (include/satmvs.h, "Facets"): T = floor(256 tol), tol [m] the distance a cell may lie off its
    neighbours' plane; Ax = floor(2048 slope_tol xres), Ay = floor(2048 slope_tol yres), slope_tol the difference of tan(slope)
    two linked cells may have per axis.  The defaults are chosen on a synthetic roof scene, not tuned on real data."""
    _grid_checked(grid, "grid")
    tol, slope_tol = float(tol), float(slope_tol)
    if not (math.isfinite(tol) and tol >= 0.0) or not (math.isfinite(slope_tol) and slope_tol >= 0.0):
        raise ValueError("tol and slope_tol must be finite and >= 0, got %r, %r" % (tol, slope_tol))
    return (_facet_term(256.0 * tol, "256 tol"), _facet_term(2048.0 * slope_tol * float(grid.xres), "2048 slope_tol xres"),
            _facet_term(2048.0 * slope_tol * float(grid.yres), "2048 slope_tol yres"))


def _facet_inputs(dsm, grid, mask):
    """The DSM (float32, never converted) and the mask (or None) on one device, checked before any device work."""
    dsm = _dsm_bits(dsm)
    if grid is not None:
        _on_grid(dsm, _grid_checked(grid, "grid"))
    if mask is not None:
        mask = _mask_checked(mask)
        if tuple(mask.shape) != tuple(dsm.shape):
            raise ValueError("mask shape %s differs from the DSM's %s" % (tuple(mask.shape), tuple(dsm.shape)))
        if not isinstance(mask, torch.Tensor):
            mask = np.not_equal(mask, 0).view(np.uint8)
    z, as_numpy = _to_device(dsm)
    m = None
    if mask is not None:
        m = (_to_device(mask, dev=z.device)[0] != 0).to(torch.uint8).contiguous()
    return z, m, as_numpy


def local_planes(dsm, grid=None, tol=0.25, mask=None, nodata=-999.0):
    """The 3 x 3 integer gradient of every cell and whether its window is planar within tol (include/satmvs.h
    smvs_dsm_facet_normals): heights q = rn(256 z); Gx, Gy int32 = 8 x the height step per column and per row (rows grow
    southwards) in units of 2^-8 m, 0 where a cell of the window is off the grid, invalid or outside `mask`; planar uint8.
    -> (Gx, Gy, planar), each (gh, gw); numpy if the DSM came as numpy, device tensors otherwise."""
    tol = float(tol)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0, got %r" % tol)
    T = _facet_term(256.0 * tol, "256 tol")
    z, m, as_numpy = _facet_inputs(dsm, grid, mask)
    gh, gw = z.shape
    Gx = torch.empty((gh, gw), dtype=torch.int32, device=z.device)
    Gy = torch.empty_like(Gx)
    planar = torch.empty((gh, gw), dtype=torch.uint8, device=z.device)
    _call(z.device, "smvs_dsm_facet_normals", z, m, gw, gh, float(nodata), T, Gx, Gy, planar)
    return _back(as_numpy, Gx, Gy, planar)


def facets(dsm, grid, tol=0.25, slope_tol=0.1, connectivity=8, grow=True, mask=None, nodata=-999.0):
    """Planar facets of a DSM (include/satmvs.h smvs_dsm_facet_label, DESIGN.md section 9, "Facets"): a cell is planar if its 3
    x 3 window lies within tol of the window's plane; two planar neighbours are linked if their gradients differ by at most
    slope_tol per axis and the step between them fits both planes within tol; a facet is a class of the transitive closure of
    links, numbered 1 .. n in raster order of its first planar cell.  With grow, one round gives a face its rim back: a valid
    cell that is not planar joins the first neighbouring planar cell whose plane passes within tol of it.  Cells outside `mask`
    (bool or integer, non-zero = inside) count as invalid.  Links are pairwise, so a gently curved surface chains into one
    facet: reject by rms_m and max_abs_m of facet_planes().  A face needs a cell whose whole 3 x 3 window lies in it.  Integer
    arithmetic throughout: the result depends on the inputs alone, bit for bit.
    -> (labels (gh, gw) int32, n int); labels numpy if the DSM came as numpy, a device tensor otherwise.  Reading n is the one
    synchronisation."""
    T, Ax, Ay = facet_terms(grid, tol, slope_tol)
    connectivity = _connectivity_checked(connectivity)
    z, m, as_numpy = _facet_inputs(dsm, grid, mask)
    gh, gw = z.shape
    nbytes = _lib.load().smvs_dsm_facet_workspace_bytes(gw, gh)
    if nbytes == 0:
        raise ValueError("unsupported facet labelling: %d x %d cells" % (gw, gh))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    labels = torch.empty((gh, gw), dtype=torch.int32, device=z.device)
    n_dev = torch.empty(1, dtype=torch.int32, device=z.device)
    _call(z.device, "smvs_dsm_facet_label", z, m, gw, gh, float(nodata), T, Ax, Ay, connectivity, int(bool(grow)), labels, n_dev, ws, nbytes)
    n = int(n_dev.item())
    if n < 0:
        raise _lib.SatMVSNativeError("smvs_dsm_facet_label gave up: a union-find loop reached its bound (n = %d)" % n)
    return _back(as_numpy, labels), n


def facet_planes(labels, n, dsm, grid=None, nodata=-999.0):
    """The least-squares plane of every label 1 .. n over its valid cells (include/satmvs.h smvs_dsm_facet_planes): exact int64
    moments about an integer centre, the plane in float64 in a fixed operation order, and its residuals.  At most 32768 cells a
    side and fewer than 2^24 cells (larger scenes go through tiles).  -> dict of arrays of length n, entry k for label k + 1:
      n_cells int64; sums int64 (n, 3): sum col, sum row, sum q (q = rn(256 z)); centre int32 (n, 2) row, col and centre_q int32,
      the floors of the means; moments int64 (n, 8): FACET_MOMENTS about the centre; plane float64 (n, 3): a [units per column], b
      [units per row], h0 [units at the centre], NaN for fewer than three cells or cells on one line; sse int64 and max_abs
      int32 of e = q - rn(plane), rms_m = sqrt(sse / n_cells) / 256 and max_abs_m (NaN with the plane)
      with grid: dzde = a / (256 xres), dzdn = -b / (256 yres); slope_deg; aspect_deg in aspect()'s convention (downslope,
      clockwise from north, NaN where both components are 0); area_m2; surface_m2 = area_m2 sqrt(1 + dzde^2 + dzdn^2); mean_m.
    Equal bits from run to run.  The dict goes into outlines() / write_geojson() as it is (NaN is written as null).  numpy if the
    labels came as numpy, device tensors otherwise."""
    labels = _labels_checked(labels)
    n = _label_count_checked(n)
    dsm = _dsm_bits(dsm)
    if tuple(dsm.shape) != tuple(labels.shape):
        raise ValueError("dsm shape %s differs from the labels' %s" % (tuple(dsm.shape), tuple(labels.shape)))
    gh, gw = int(labels.shape[0]), int(labels.shape[1])
    if gw > MAX_FACET_PLANE_SIDE or gh > MAX_FACET_PLANE_SIDE or gw * gh >= MAX_FACET_PLANE_CELLS:
        raise ValueError("facet_planes takes at most 32768 cells a side and fewer than 2^24 cells, got %d x %d" % (gh, gw))
    if grid is not None:
        _on_grid(labels, _grid_checked(grid, "grid"))
    lab, as_numpy = _to_device(labels)
    dev = lab.device
    z, _ = _to_device(dsm, dev=dev)
    sums = torch.empty((n, 4), dtype=torch.int64, device=dev)
    centre = torch.empty((n, 3), dtype=torch.int32, device=dev)
    moments = torch.empty((n, 8), dtype=torch.int64, device=dev)
    plane = torch.empty((n, 3), dtype=torch.float64, device=dev)
    sse = torch.empty(n, dtype=torch.int64, device=dev)
    max_abs = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        _call(dev, "smvs_dsm_facet_planes", lab, z, gw, gh, float(nodata), n, sums, centre, moments, plane, sse, max_abs)
    cells = sums[:, 0]
    nan = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    fitted = ~torch.isnan(plane[:, 2])
    per_cell = cells.double().clamp(min=1.0)
    out = {"n_cells": cells, "sums": sums[:, 1:], "centre": torch.stack([centre[:, 1], centre[:, 0]], dim=1), "centre_q": centre[:, 2],
           "moments": moments, "plane": plane, "sse": sse, "max_abs": max_abs,
           "rms_m": torch.where(fitted, torch.sqrt(sse.double() / per_cell) / 256.0, nan),
           "max_abs_m": torch.where(fitted, max_abs.double() / 256.0, nan)}
    if grid is not None:
        # tensor divisors: a division by a Python scalar is a multiplication by its rounded reciprocal on the device
        dzde = plane[:, 0] / torch.full_like(nan, 256.0 * float(grid.xres))
        dzdn = -plane[:, 1] / torch.full_like(nan, 256.0 * float(grid.yres))
        asp = torch.rad2deg(torch.atan2(-dzde, -dzdn))
        asp = torch.where(asp < 0.0, asp + 360.0, asp)
        asp = torch.where(asp >= 360.0, torch.zeros_like(asp), asp)
        area = cells.double() * float(grid.xres) * float(grid.yres)
        out.update({"dzde": dzde, "dzdn": dzdn, "slope_deg": torch.rad2deg(torch.atan(torch.sqrt(dzde * dzde + dzdn * dzdn))),
                    "aspect_deg": torch.where((dzde == 0.0) & (dzdn == 0.0), nan, asp), "area_m2": area,
                    "surface_m2": area * torch.sqrt(1.0 + dzde * dzde + dzdn * dzdn),
                    "mean_m": torch.where(cells > 0, sums[:, 3].double() / per_cell / 256.0, nan)})
    return {k: _back(as_numpy, t) for k, t in out.items()}


def extract_roofs(dsm, above, grid, min_height=2.5, min_area_m2=50.0, facet_min_area_m2=25.0, max_rms=None, tol=0.25, slope_tol=0.1,
                  nodata=-999.0):
    """The roof faces of a DSM: extract_objects(above, grid, min_height, min_area_m2) -> facets(dsm, mask = objects > 0) ->
    facet_planes() -> sieve_labels() at ceil(facet_min_area_m2 / (xres yres)) cells and, with max_rms [m], at rms_m <= max_rms (a
    facet without a plane goes with it).  `above` is the nDSM of `dsm` (ndsm()).  The defaults are chosen on a synthetic roof
    scene, not tuned on real data.  -> (labels (gh, gw) int32 with 1 .. n' on the facets that stay, table: the dict of
    facet_planes(grid=grid) restricted to them, and `object` int32 = the label of extract_objects under each facet's first
    cell); numpy if the DSM came as numpy, device tensors otherwise."""
    dsm = _on_grid(_dsm_bits(dsm), _grid_checked(grid, "grid"))
    facet_terms(grid, tol, slope_tol)                        # rejected here, before any device work
    facet_min_area_m2 = float(facet_min_area_m2)
    if not (math.isfinite(facet_min_area_m2) and facet_min_area_m2 >= 0.0):
        raise ValueError("facet_min_area_m2 must be finite and >= 0, got %r" % facet_min_area_m2)
    if max_rms is not None:
        max_rms = float(max_rms)
        if not (math.isfinite(max_rms) and max_rms >= 0.0):
            raise ValueError("max_rms must be finite and >= 0, got %r" % max_rms)
    min_cells = _int_checked(int(math.ceil(facet_min_area_m2 / (float(grid.xres) * float(grid.yres)))), "facet_min_area_m2 in cells", 0, 2 ** 31 - 1)
    z, as_numpy = _to_device(dsm)
    a, _ = _to_device(_dsm_bits(above), dev=z.device)
    objects, _ = extract_objects(a, grid, min_height, min_area_m2, nodata=nodata)
    labels, n = facets(z, grid, tol, slope_tol, mask=objects > 0, nodata=nodata)
    table = facet_planes(labels, n, z, grid, nodata)
    size = table["n_cells"].to(torch.int32)
    if max_rms is not None:
        size = torch.where(table["rms_m"] <= max_rms, size, torch.zeros_like(size))
    labels, _, kept = sieve_labels(labels, size, max(min_cells, 1))
    table = {k: t[kept] for k, t in table.items()}
    cell = torch.arange(labels.numel(), dtype=torch.int64, device=z.device)
    first = torch.full((len(kept) + 1,), labels.numel(), dtype=torch.int64, device=z.device)
    first.scatter_reduce_(0, labels.reshape(-1).long(), cell, reduce="amin")
    table["object"] = objects.reshape(-1)[first[1:]] if len(kept) else torch.zeros(0, dtype=torch.int32, device=z.device)
    return _back(as_numpy, labels), {k: _back(as_numpy, t) for k, t in table.items()}


# ---- zonal order statistics: medians, percentiles and NMAD per label -------------------------------------------------------------
MAX_SELECT_RANKS = 8                                              # slots of one smvs_dsm_label_select call
MAX_SELECT_SLOTS = 2 ** 28                                        # n * n_ranks stays below it
MAX_QUANTILE_DEN = 1 << 16
QUANTILE_METHODS = ("linear", "lower", "higher", "midpoint", "nearest")
NMAD_FACTOR = 1.4826                                              # MAD -> the standard deviation of a normal distribution


def _quantile_fractions(q):
    """The quantile levels as reduced (num, den) pairs: each a Fraction, a (num, den) pair of integers, or a float taken as
    Fraction(q).limit_denominator(2^16); 0 <= q <= 1 and den <= 2^16 after reduction."""
    from fractions import Fraction
    if isinstance(q, (Fraction, float, int, np.floating, np.integer)) and not isinstance(q, bool):
        q = (q,)
    if isinstance(q, (np.ndarray, torch.Tensor)):
        q = [float(v) for v in q.reshape(-1).tolist()]
    if not isinstance(q, (list, tuple)) or len(q) == 0:
        raise ValueError("q is a non-empty sequence of quantile levels, got %r" % (q,))
    out = []
    for v in q:
        if isinstance(v, Fraction):
            f = v
        elif isinstance(v, (tuple, list)):
            if len(v) != 2 or any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) for t in v) or int(v[1]) <= 0:
                raise ValueError("a quantile level given as a pair is (num, den) of integers with den > 0, got %r" % (v,))
            f = Fraction(int(v[0]), int(v[1]))
        elif isinstance(v, (float, int, np.floating, np.integer)) and not isinstance(v, bool):
            if not math.isfinite(float(v)):
                raise ValueError("a quantile level must be finite, got %r" % (v,))
            f = Fraction(v if isinstance(v, int) else float(v)).limit_denominator(MAX_QUANTILE_DEN)
        else:
            raise ValueError("a quantile level is a Fraction, a (num, den) pair or a float, got %r" % (v,))
        if not 0 <= f <= 1:
            raise ValueError("a quantile level must be in [0, 1], got %r" % (v,))
        if f.denominator > MAX_QUANTILE_DEN:
            raise ValueError("a quantile level's denominator must be at most 2^16 after reduction, got %r" % (v,))
        out.append((f.numerator, f.denominator))
    return out


def quantile_ranks(n_valid, q):
    """The two ranks a quantile lies between, in integers: with m = n_valid and q = num / den, h = (m - 1) num (int64),
    lo = h // den, rem = h % den, hi = lo + (rem > 0): the quantile is the order statistic lo, or lies rem / den of the way to
    the order statistic hi.  m = 0 gives lo = hi = -1, rem = 0.  n_valid (n) of an integer dtype with 0 <= m < 2^31, numpy or a
    tensor on any device (no device needed); q as in label_quantiles.
    -> (lo int32 (n, Q), hi int32 (n, Q), rem int64 (n, Q), den int64 (Q)), of n_valid's kind."""
    fr = _quantile_fractions(q)
    is_tensor = isinstance(n_valid, torch.Tensor)
    m = n_valid if is_tensor else np.asarray(n_valid)
    integral = not (m.is_floating_point() or m.is_complex() or m.dtype == torch.bool) if is_tensor else np.issubdtype(m.dtype, np.integer)
    if m.ndim != 1 or not integral:
        raise ValueError("n_valid is a 1-D integer array, one entry per label, got %s %s" % (m.dtype, tuple(m.shape)))
    if is_tensor:
        m64 = m.to(torch.int64)[:, None]
        num = torch.tensor([f[0] for f in fr], dtype=torch.int64, device=m.device)
        den = torch.tensor([f[1] for f in fr], dtype=torch.int64, device=m.device)
        some = m64 > 0
        h = (m64 - 1).clamp(min=0) * num
        lo = torch.div(h, den, rounding_mode="floor")
        rem = h - lo * den
        hi = lo + (rem > 0)
        none = torch.full_like(lo, -1)
        return torch.where(some, lo, none).to(torch.int32), torch.where(some, hi, none).to(torch.int32), rem, den
    if m.size and (int(m.min()) < 0 or int(m.max()) >= 2 ** 31):
        raise ValueError("n_valid must be in 0 .. 2^31 - 1")
    m64 = m.astype(np.int64)[:, None]
    num = np.array([f[0] for f in fr], dtype=np.int64)
    den = np.array([f[1] for f in fr], dtype=np.int64)
    some = m64 > 0
    h = np.maximum(m64 - 1, 0) * num
    lo = h // den
    rem = h - lo * den
    hi = lo + (rem > 0)
    return np.where(some, lo, -1).astype(np.int32), np.where(some, hi, -1).astype(np.int32), rem, den


def _quantile_value(lo, hi, lo_rank, rem, den, method):
    """The quantile in float64 from its two order statistics (float32 tensors) by `method`; the operation order is the rule."""
    a, b = lo.double(), hi.double()
    if method == "lower":
        return a
    if method == "higher":
        return b
    if method == "midpoint":
        return (a + b) * 0.5
    if method == "nearest":
        upper = (2 * rem > den) | ((2 * rem == den) & (lo_rank % 2 == 1))       # on a tie the one of even rank
        return torch.where(upper, b, a)
    return a + (b - a) * (rem.double() / den.double())                          # tensor divisor: a true division on the device


def _label_select(lab, v, n, nodata, centre, ranks):
    """smvs_dsm_label_select over the columns of ranks (n, S) int32 in chunks of 8 -> out (n, S) float32."""
    dev = lab.device
    gh, gw = lab.shape
    S = int(ranks.shape[1])
    out = torch.empty((n, S), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    width = min(S, MAX_SELECT_RANKS)
    nbytes = _lib.load().smvs_dsm_label_select_workspace_bytes(n, width)
    if nbytes == 0:
        raise ValueError("unsupported selection: %d labels x %d ranks (n * n_ranks must be below 2^28)" % (n, width))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for s0 in range(0, S, MAX_SELECT_RANKS):
        r = ranks[:, s0:s0 + MAX_SELECT_RANKS].contiguous()
        o = torch.empty(r.shape, dtype=torch.float32, device=dev)
        _call(dev, "smvs_dsm_label_select", lab, v, gw, gh, nodata, n, centre, r, int(r.shape[1]), o, None, ws, nbytes)
        out[:, s0:s0 + MAX_SELECT_RANKS] = o
    return out


def label_quantiles(labels, n, values, q=(0.5,), method="linear", centre=None, nodata=-999.0):
    """Exact quantiles of the values under every label 1 .. n (include/satmvs.h smvs_dsm_label_select, DESIGN.md section 9, "Zonal
    order statistics"): labels (gh, gw) int32, any zone map (label(), facets(), burn_polygons(), a class grid); values (gh, gw)
    float32, never converted; a cell counts iff its label is in 1 .. n and its value is finite and != nodata.  q: the levels,
    each a Fraction, a (num, den) pair or a float taken as Fraction(q).limit_denominator(2^16).  With centre ((n) float32) the
    statistics are those of |value - centre[k]| (float64 difference, rounded to float32 once); a label whose centre is not finite
    has no cell.  -> dict, entry k for label k + 1:
      n_valid int32 (n): the cells that count
      lo, hi float32 (n, Q): the order statistics of quantile_ranks(), input values with their own bits (order: -0.0 below +0.0);
        nodata where n_valid is 0
      value float64 (n, Q), NaN where n_valid is 0, by `method`: "linear" lo + (hi - lo) (rem / den), "lower", "higher",
        "midpoint" (lo + hi) 0.5, "nearest" (the closer rank, on a tie the even one)
    Selection, no sums: equal bits from run to run.  numpy if the labels came as numpy, device tensors otherwise."""
    labels = _labels_checked(labels)
    n = _label_count_checked(n)
    values = _dsm_bits(values)
    if tuple(values.shape) != tuple(labels.shape):
        raise ValueError("values shape %s differs from the labels' %s" % (tuple(values.shape), tuple(labels.shape)))
    fr = _quantile_fractions(q)
    if method not in QUANTILE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (QUANTILE_METHODS, method))
    if centre is not None:
        if not isinstance(centre, torch.Tensor):
            centre = np.asarray(centre)
        if centre.ndim != 1 or int(centre.shape[0]) != n or centre.dtype not in (np.float32, torch.float32):
            raise ValueError("centre is float32 (n) with n = %d, got %s %s" % (n, centre.dtype, tuple(centre.shape)))
    if n * min(2 * len(fr), MAX_SELECT_RANKS) >= MAX_SELECT_SLOTS:
        raise ValueError("too many labels for one selection: n * n_ranks must be below 2^28, got n = %d" % n)
    lab, as_numpy = _to_device(labels)
    dev = lab.device
    v, _ = _to_device(values, dev=dev)
    c = None if centre is None else _to_device(centre, dev=dev)[0]
    nd = float(nodata)
    gh, gw = lab.shape
    m = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:                                                    # the cells that count, before any rank can be named
        area = torch.empty(n, dtype=torch.int32, device=dev)
        bbox = torch.empty((n, 4), dtype=torch.int32, device=dev)
        rc = torch.empty((n, 2), dtype=torch.int64, device=dev)
        vmin = torch.empty(n, dtype=torch.float32, device=dev)
        vmax = torch.empty_like(vmin)
        qsum = torch.empty(n, dtype=torch.int64, device=dev)
        _call(dev, "smvs_dsm_label_stats", lab, v, gw, gh, nd, n, area, bbox, rc, m, vmin, vmax, qsum)
        if c is not None:
            m = torch.where(torch.isfinite(c), m, torch.zeros_like(m))
    lo_rank, hi_rank, rem, den = quantile_ranks(m, fr)
    split = [f[0] % f[1] != 0 for f in fr]                   # q = 0 and q = 1 never lie between two ranks
    cols = [lo_rank[:, i] for i in range(len(fr))] + [hi_rank[:, i] for i in range(len(fr)) if split[i]]
    got = _label_select(lab, v, n, nd, c, torch.stack(cols, dim=1))
    lo = got[:, :len(fr)].contiguous()
    hi = lo.clone()
    at = len(fr)
    for i in range(len(fr)):
        if split[i]:
            hi[:, i] = got[:, at]
            at += 1
    value = _quantile_value(lo, hi, lo_rank, rem, den, method)
    value = torch.where((m > 0)[:, None], value, torch.full_like(value, float("nan")))
    return {k: _back(as_numpy, t) for k, t in (("n_valid", m), ("lo", lo), ("hi", hi), ("value", value))}


def label_nmad(labels, n, values, nodata=-999.0):
    """The robust centre and spread of the values under every label: median float64 (n), the linear median of
    label_quantiles(); mad float64, the linear median of |value - float32(median)| (label_quantiles with centre); nmad =
    1.4826 mad, the standard deviation of a normal distribution with that MAD; n_valid int32.  NaN where n_valid is 0.
    numpy if the labels came as numpy, device tensors otherwise."""
    from fractions import Fraction
    as_numpy = not isinstance(labels, torch.Tensor)
    half = (Fraction(1, 2),)
    first = label_quantiles(labels, n, values, half, "linear", None, nodata)
    median = torch.as_tensor(first["value"])[:, 0]
    centre = median.to(torch.float32)
    second = label_quantiles(labels, n, values, half, "linear", centre.numpy() if as_numpy else centre, nodata)
    mad = torch.as_tensor(second["value"])[:, 0]
    out = {"median": median, "mad": mad, "nmad": mad * NMAD_FACTOR, "n_valid": torch.as_tensor(first["n_valid"])}
    return {k: (t.cpu().numpy() if as_numpy else t) for k, t in out.items()}


# ---- focal statistics: exact summed-area tables, any window in O(1) per cell ---------------------------------------------------
MAX_FOCAL_RECTS = 1024                                            # records of one window
MAX_FOCAL_OFFSET = 4096                                           # cells a record may reach from the centre
MAX_FOCAL_AREA = 1 << 24                                          # W+, the cells of a window's positive rectangles
FOCAL_SHAPES = ("box", "disc", "annulus")


@dataclass(frozen=True)
class FocalWindow:
    """A window as a signed sum of rectangles: rects (k, 5) int32 records {dx0, dx1, dy0, dy1, sign}, bounds inclusive;
    cells, the cells of the window; positive, W+, the cells of the records with sign +1 (what the overflow bound counts)."""
    rects: np.ndarray
    cells: int
    positive: int


def _half_widths(radius, xres, yres, box=False):
    """hx[k], k = 0 .. 2 ky, of row dy = k - ky: the largest dx >= 0 that belongs, -1 where none does.  Disc: (dx xres)^2 +
    (dy yres)^2 <= radius^2 in float64 in that order; box: |dx xres| <= radius and |dy yres| <= radius."""
    kx, ky = int(radius / xres) + 1, int(radius / yres) + 1
    if max(kx, ky) > 2 * MAX_FOCAL_OFFSET:                   # the exact test below is quadratic in these
        raise ValueError("a window reaches at most %d cells from its centre, got radius %r at cells of %r x %r" % (MAX_FOCAL_OFFSET, radius, xres, yres))
    dx = np.arange(0, kx + 1, dtype=np.float64) * np.float64(xres)
    dy = np.arange(-ky, ky + 1, dtype=np.float64) * np.float64(yres)
    if box:
        inside = (np.abs(dx)[None, :] <= radius) & (np.abs(dy)[:, None] <= radius)
    else:
        inside = (dx * dx)[None, :] + (dy * dy)[:, None] <= np.float64(radius) * np.float64(radius)
    hx = inside.sum(axis=1).astype(np.int64) - 1             # the test is monotone in dx, so the members are 0 .. hx
    return hx, ky


def _disc_records(radius, xres, yres, sign, box=False):
    hx, ky = _half_widths(radius, xres, yres, box)
    rows = np.flatnonzero(hx >= 0)
    if rows.size == 0:
        return np.zeros((0, 5), dtype=np.int64), 0
    cells = int((2 * hx[rows] + 1).sum())
    out = []
    start = rows[0]
    for k in range(rows[0], rows[-1] + 1):                   # rows of equal extent side by side are one record
        if k == rows[-1] or hx[k + 1] != hx[start]:
            out.append((-hx[start], hx[start], start - ky, k - ky, sign))
            start = k + 1
    return np.array(out, dtype=np.int64), cells


def _focal_records_checked(rects):
    r = np.asarray(rects)
    if r.ndim != 2 or r.shape[1] != 5 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("window records are (k, 5) integers {dx0, dx1, dy0, dy1, sign}, got %s %s" % (r.dtype, tuple(r.shape)))
    if not 1 <= r.shape[0] <= MAX_FOCAL_RECTS:
        raise ValueError("a window has 1 .. %d records, got %d" % (MAX_FOCAL_RECTS, r.shape[0]))
    r = r.astype(np.int64)
    if np.abs(r[:, :4]).max() > MAX_FOCAL_OFFSET:
        raise ValueError("a window reaches at most %d cells from its centre" % MAX_FOCAL_OFFSET)
    if (r[:, 0] > r[:, 1]).any() or (r[:, 2] > r[:, 3]).any() or (np.abs(r[:, 4]) != 1).any():
        raise ValueError("a window record has dx0 <= dx1, dy0 <= dy1 and sign +1 or -1")
    area = (r[:, 1] - r[:, 0] + 1) * (r[:, 3] - r[:, 2] + 1)
    positive = int(area[r[:, 4] > 0].sum())
    if positive > MAX_FOCAL_AREA:
        raise ValueError("a window's positive records hold at most 2^24 cells, got %d" % positive)
    return FocalWindow(np.ascontiguousarray(r, dtype=np.int32), int((area * r[:, 4]).sum()), positive)


def focal_window(shape, radius, inner=None, grid=None):
    """The window of the focal operators as rectangle records (include/satmvs.h smvs_dsm_focal_query): shape "box", "disc" or
    "annulus"; radius (and inner) in cells without a grid and in metres with one.  Cell (dx, dy) belongs to a disc iff
    (dx xres)^2 + (dy yres)^2 <= radius^2 in float64 in that order (an ellipse in cells where xres != yres), to a box iff
    |dx xres| <= radius and |dy yres| <= radius, to an annulus iff it belongs to the disc and (dx xres)^2 + (dy yres)^2 >
    inner^2: the disc of `radius` minus the disc of `inner`, 0 <= inner < radius.  Rows of equal extent are one record.
    -> FocalWindow(rects (k, 5) int32, cells, positive = W+).  Host code, numpy only."""
    if shape not in FOCAL_SHAPES:
        raise ValueError("shape must be one of %s, got %r" % (FOCAL_SHAPES, shape))
    radius = _finite(radius, "radius")
    if radius < 0.0:
        raise ValueError("radius must be >= 0, got %r" % radius)
    if (inner is not None) != (shape == "annulus"):
        raise ValueError("inner goes with the annulus and with it alone")
    xres, yres = (1.0, 1.0) if grid is None else (float(_grid_checked(grid, "grid").xres), float(grid.yres))
    rects, _ = _disc_records(radius, xres, yres, 1, box=shape == "box")
    if shape == "annulus":
        inner = _finite(inner, "inner")
        if not 0.0 <= inner < radius:
            raise ValueError("inner must be in [0, radius), got %r" % inner)
        rects = np.concatenate([rects, _disc_records(inner, xres, yres, -1)[0]])
    if rects.shape[0] == 0:
        raise ValueError("the window holds no cell")
    return _focal_records_checked(rects)


def _window_checked(window):
    """A FocalWindow as it is (focal_window() has checked it); bare records are checked and counted."""
    return window if isinstance(window, FocalWindow) else _focal_records_checked(window)


class FocalTables:
    """The summed-area tables of one DSM (focal_tables()): the device buffer, the sizes, and the header read back once: qmin,
    qmax [2^-8 m], n_valid, centre (the height sums are measured from) and max_abs (D, the largest |q - centre|)."""

    def __init__(self, buffer, width, height, header, as_numpy):
        self.buffer, self.width, self.height, self.as_numpy = buffer, width, height, as_numpy
        self.qmin, self.qmax, self.n_valid, self.centre, self.max_abs = (int(v) for v in header[:5])

    def check(self, window):
        """ValueError where the window's sums may wrap: W+ max_abs^2 >= 2^63, in Python integers; no read of the device."""
        if window.positive * self.max_abs * self.max_abs >= 2 ** 63:
            raise ValueError("the window's sums may wrap: %d cells x (%d / 256 m)^2 >= 2^63; take a smaller window or a DSM of a "
                             "narrower height range" % (window.positive, self.max_abs))


def focal_tables(dsm, nodata=-999.0):
    """The exact summed-area tables of a DSM (include/satmvs.h smvs_dsm_focal_build, DESIGN.md section 9, "Focal statistics"):
    computed once, they serve any number of windows at any radius in O(1) per cell.  dsm (gh, gw) float32, never converted, with
    (gw + 1) (gh + 1) < 2^31; a cell is valid iff finite, != nodata and |z| <= 32768.  -> FocalTables (one read of the device:
    the header)."""
    dsm = _dsm_bits(dsm)
    gh, gw = int(dsm.shape[0]), int(dsm.shape[1])
    if (gw + 1) * (gh + 1) >= 2 ** 31:
        raise ValueError("focal tables need (gw + 1) (gh + 1) < 2^31, got %d x %d" % (gw, gh))
    z, as_numpy = _to_device(dsm)
    nbytes = _lib.load().smvs_dsm_focal_table_bytes(gw, gh)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    _call(z.device, "smvs_dsm_focal_build", z, gw, gh, float(nodata), buf, nbytes)
    return FocalTables(buf, gw, gh, buf[:64].view(torch.int64).cpu().tolist(), as_numpy)


def _focal_query(tables, window, stride=(1, 1), origin=(0, 0), shape=None, min_valid=1, sums=True, moments=True):
    """One smvs_dsm_focal_query: stride (sy, sx), origin (r0, c0), shape (oh, ow) (None: every centre from the origin on).
    -> (n, s1, s2, mean, var) device tensors, None where not asked for."""
    if not isinstance(tables, FocalTables):
        raise ValueError("tables come from focal_tables(), got %r" % type(tables).__name__)
    window = _window_checked(window)
    tables.check(window)
    sy, sx = _int_pair(stride, "stride")
    r0, c0 = _int_pair(origin, "origin")
    gw, gh = tables.width, tables.height
    if sx < 1 or sy < 1 or not (0 <= r0 < gh and 0 <= c0 < gw):
        raise ValueError("stride must be >= 1 and the origin a cell of the grid, got stride %r, origin %r" % (stride, origin))
    oh, ow = ((gh - 1 - r0) // sy + 1, (gw - 1 - c0) // sx + 1) if shape is None else _int_pair(shape, "shape")
    if oh < 1 or ow < 1 or r0 + (oh - 1) * sy > gh - 1 or c0 + (ow - 1) * sx > gw - 1:
        raise ValueError("every output centre must lie inside the grid, got shape %r" % ((oh, ow),))
    min_valid = _int_checked(min_valid, "min_valid", 0, 2 ** 31 - 1)
    dev = tables.buffer.device
    new = lambda dtype: torch.empty((oh, ow), dtype=dtype, device=dev)
    n, s1, s2 = (new(torch.int32), new(torch.int64), new(torch.int64)) if sums else (None, None, None)
    mean, var = (new(torch.float64), new(torch.float64)) if moments else (None, None)
    status = torch.empty(1, dtype=torch.int32, device=dev)   # the host check above already answered it: never read
    _call(dev, "smvs_dsm_focal_query", tables.buffer, gw, gh, window.rects, int(window.rects.shape[0]), ow, oh, c0, r0, sx, sy,
          min_valid, n, s1, s2, mean, var, status)
    return n, s1, s2, mean, var


def focal_sums(tables, window, stride=(1, 1), origin=(0, 0), shape=None):
    """The exact integers of every cell's window: n int32 the valid cells, s1 int64 the sum of q - centre, s2 int64 the sum of
    (q - centre)^2 (below 2^63: focal_tables' check), q the heights in units of 2^-8 m; centre, a Python int.  Output cell
    (R, C) sits at input cell (origin + (R, C) * stride); rectangles are clipped to the grid.  -> dict; numpy if the tables'
    DSM came as numpy, device tensors otherwise."""
    n, s1, s2, _, _ = _focal_query(tables, window, stride, origin, shape, moments=False)
    out = dict(zip(("n", "s1", "s2"), _back(tables.as_numpy, n, s1, s2)))
    out["centre"] = tables.centre
    return out


def _focal_tables_of(dsm_or_tables, nodata):
    return dsm_or_tables if isinstance(dsm_or_tables, FocalTables) else focal_tables(dsm_or_tables, nodata)


def _focal_stats(tables, window, min_valid, stride=(1, 1)):
    n, _, _, mean, var = _focal_query(tables, window, stride, min_valid=min_valid)
    return n, mean, var


def focal_stats(dsm_or_tables, window, min_valid=1, nodata=-999.0):
    """Mean and spread of every cell's window (smvs_dsm_focal_query): n int32; mean [m] and var [m^2] float64 in the entry's
    fixed order of operations, the population variance; std = sqrt(var).  NaN where n < max(min_valid, 1).  dsm_or_tables: a
    DSM (tables are built and dropped) or focal_tables() of one (nodata is then the tables').  -> dict."""
    tables = _focal_tables_of(dsm_or_tables, nodata)
    n, mean, var = _focal_stats(tables, window, min_valid)
    return dict(zip(("n", "mean", "var", "std"), _back(tables.as_numpy, n, mean, var, torch.sqrt(var))))


def _focal_valid(z, nodata):
    return _valid_cells(z, nodata) & (z.abs() <= 32768.0)


def _focal_grid(value, keep, nodata):
    """(float)value where `keep` and the value is a number, nodata elsewhere."""
    keep = keep & ~torch.isnan(value)
    return torch.where(keep, value.float(), torch.full(value.shape, float(nodata), dtype=torch.float32, device=value.device))


def focal_mean(dsm, window, min_valid=1, nodata=-999.0, tables=None):
    """The DSM smoothed by a focal mean: (float)mean of focal_stats(), nodata where n < max(min_valid, 1).  tables: focal_tables()
    of this DSM, to share them between calls.  -> (gh, gw) float32."""
    tables = tables or focal_tables(dsm, nodata)
    n, mean, _ = _focal_stats(tables, window, min_valid)
    return _back(tables.as_numpy, _focal_grid(mean, n >= min_valid, nodata))


def roughness(dsm, window, min_valid=1, nodata=-999.0, tables=None):
    """The standard deviation of the heights in every cell's window [m]: (float)sqrt(var) of focal_stats(), nodata where
    n < max(min_valid, 1).  -> (gh, gw) float32."""
    tables = tables or focal_tables(dsm, nodata)
    n, _, var = _focal_stats(tables, window, min_valid)
    return _back(tables.as_numpy, _focal_grid(torch.sqrt(var), n >= min_valid, nodata))


def _tpi(dsm, grid, radius, inner, min_valid, nodata, tables):
    _on_grid(_dsm_bits(dsm), _grid_checked(grid, "grid"))
    window = focal_window("disc" if inner is None else "annulus", radius, inner, grid)
    tables = tables or focal_tables(dsm, nodata)
    z, as_numpy = _to_device(dsm, dev=tables.buffer.device)
    n, mean, var = _focal_stats(tables, window, min_valid)
    return as_numpy, z.double() - mean, torch.sqrt(var), _focal_valid(z, nodata) & (n >= min_valid)


def tpi(dsm, grid, radius, inner=None, min_valid=1, nodata=-999.0, tables=None):
    """The topographic position index: (float)((double)z - mean) with the mean over a disc of `radius` [m] about the cell, or
    over the annulus between `inner` and `radius` where inner is given (focal_window()); nodata where the cell itself is invalid
    or its window holds fewer than max(min_valid, 1) valid cells.  -> (gh, gw) float32."""
    as_numpy, t, _, keep = _tpi(dsm, grid, radius, inner, min_valid, nodata, tables)
    return _back(as_numpy, _focal_grid(t, keep, nodata))


def dev(dsm, grid, radius, inner=None, min_valid=1, nodata=-999.0, tables=None):
    """The deviation from mean elevation: (float)(((double)z - mean) / std) over tpi()'s window, the TPI in units of the
    window's own standard deviation; nodata where tpi() has none and where std is 0.  -> (gh, gw) float32."""
    as_numpy, t, std, keep = _tpi(dsm, grid, radius, inner, min_valid, nodata, tables)
    return _back(as_numpy, _focal_grid(t / std, keep & (std > 0.0), nodata))


def focal_fraction(mask, window):
    """The share of set cells among the cells of every cell's window that lie inside the grid: the density of a footprint
    mask (extract_objects' labels > 0) or of a validity mask.  The mask goes through the same entry as float32 0 / 1; the count
    of set cells is the integer (s1 + n centre) / 256, the share float64 count / n, NaN where the window holds no cell of the
    grid.  mask (gh, gw) bool or uint8.  -> (gh, gw) float64."""
    m, as_numpy = _to_device(_mask_checked(mask))
    tables = focal_tables((m != 0).float())
    n, s1, _, _, _ = _focal_query(tables, window, moments=False)
    n = n.to(torch.int64)
    count = (s1 + n * tables.centre) >> 8
    return _back(as_numpy, torch.where(n > 0, count.double() / n.double(), torch.full_like(count, float("nan"), dtype=torch.float64)))


def aggregate(dsm, grid, factor, min_valid=1, nodata=-999.0):
    """A block-averaged overview: cell (R, C) of the result is the focal mean over the factor x factor block whose upper-left
    cell is (R factor, C factor) (the strided query with the rectangle [0, factor - 1]^2), nodata where the block holds fewer
    than max(min_valid, 1) valid cells; a last partial block is kept and clipped.  The new grid's cell (0, 0) has its centre
    (factor - 1) / 2 cells east and south of the old one's and the resolution is multiplied by factor.
    -> (dsm (ceil(gh / factor), ceil(gw / factor)) float32, DSMGrid, count int32)."""
    _on_grid(_dsm_bits(dsm), _grid_checked(grid, "grid"))
    f = _int_checked(factor, "factor", 1, MAX_FOCAL_OFFSET + 1)
    tables = focal_tables(dsm, nodata)
    n, _, _, mean, _ = _focal_query(tables, np.array([[0, f - 1, 0, f - 1, 1]], dtype=np.int32), (f, f), min_valid=min_valid)
    coarse = DSMGrid(grid.e0 + 0.5 * (f - 1) * grid.xres, grid.n0 - 0.5 * (f - 1) * grid.yres, grid.xres * f, grid.yres * f,
                     int(n.shape[1]), int(n.shape[0]))
    out, count = _back(tables.as_numpy, _focal_grid(mean, n >= min_valid, nodata), n)
    return out, coarse, count


SLOPE_POSITIONS = ("no data", "valley", "lower slope", "flat", "middle slope", "upper slope", "ridge")


def slope_position(dsm, grid, radius, slope_deg=5.0, min_valid=1, nodata=-999.0):
    """Weiss' six slope positions from dev() over a disc of `radius` [m] and slope(): uint8 0 no data (dev or slope has none),
    1 valley (dev <= -1), 2 lower slope (-1 < dev <= -0.5), 3 flat (-0.5 < dev < 0.5, slope <= slope_deg), 4 middle slope
    (the same band, steeper), 5 upper slope (0.5 <= dev < 1), 6 ridge (dev >= 1).  dev() standardises LOCALLY, by the
    standard deviation of each cell's own window, where Weiss standardises the TPI by its standard deviation over the whole
    grid.  The defaults were chosen for 5 m grids on the synthetic scene; they are not tuned on real data.
    -> (gh, gw) uint8."""
    slope_deg = _finite(slope_deg, "slope_deg")
    as_numpy, t, std, keep = _tpi(dsm, grid, radius, None, min_valid, nodata, None)
    d = (t / std).float()
    s, _ = _to_device(slope(dsm, grid, nodata), dev=d.device)
    cls = torch.full(d.shape, 3, dtype=torch.uint8, device=d.device)
    cls[s > slope_deg] = 4
    cls[d <= -0.5] = 2
    cls[d <= -1.0] = 1
    cls[d >= 0.5] = 5
    cls[d >= 1.0] = 6
    cls[~(keep & (std > 0.0)) | torch.isnan(d) | torch.isnan(s)] = 0
    return _back(as_numpy, cls)


# ---- focal order statistics: exact moving-window medians, quantiles and counts --------------------------------------------------
MAX_RANK_RUNS = 130                                               # row runs of one window: two a row at +-32 rows
MAX_RANK_OFFSET = 32                                              # cells a window may reach from its centre
MAX_RANK_LEVELS = 4                                               # levels of one smvs_dsm_focal_select call
RANK_TILE = 32                                                    # SMVS_DSM_RANK_TILE of include/satmvs.h


def _window_runs(window):
    """The window of the focal order statistics as row runs (include/satmvs.h smvs_dsm_focal_select): (k, 3) int32 records
    {dy, dx0, dx1}, bounds inclusive, sorted by (dy, dx0), the runs of a row neither overlapping nor touching.  window: a
    FocalWindow (focal_window(): its signed rectangles are rasterised here on the host, and every cell's coverage must come out
    0 or 1, so box, disc and annulus hold exactly focal_window's cells), bare rectangle records, or a 2-D boolean footprint of
    odd sizes about its middle cell.  A window reaches at most 32 cells from its centre and has at most 130 runs."""
    if isinstance(window, FocalWindow) or not (isinstance(window, (np.ndarray, torch.Tensor)) and window.dtype in (np.bool_, torch.bool)):
        rects = _window_checked(window).rects.astype(np.int64)
        reach = int(np.abs(rects[:, :4]).max())
        if reach > MAX_RANK_OFFSET:
            raise ValueError("a window of the focal order statistics reaches at most %d cells from its centre, got %d" % (MAX_RANK_OFFSET, reach))
        cover = np.zeros((2 * reach + 1, 2 * reach + 1), dtype=np.int64)
        for dx0, dx1, dy0, dy1, sign in rects:
            cover[dy0 + reach:dy1 + reach + 1, dx0 + reach:dx1 + reach + 1] += sign
        if cover.min() < 0 or cover.max() > 1:
            raise ValueError("the window's signed rectangles must cover every cell 0 or 1 times, got a coverage of %d"
                             % (cover.max() if cover.max() > 1 else cover.min()))
        foot = cover == 1
    else:
        foot = window.cpu().numpy() if isinstance(window, torch.Tensor) else window
        if foot.ndim != 2 or foot.shape[0] % 2 != 1 or foot.shape[1] % 2 != 1:
            raise ValueError("a footprint is a 2-D boolean array of odd sizes, got shape %s" % (tuple(foot.shape),))
        if max(foot.shape) // 2 > MAX_RANK_OFFSET and (np.abs(np.argwhere(foot) - np.array(foot.shape) // 2) > MAX_RANK_OFFSET).any():
            raise ValueError("a window of the focal order statistics reaches at most %d cells from its centre" % MAX_RANK_OFFSET)
    ky, kx = foot.shape[0] // 2, foot.shape[1] // 2
    runs = []
    for row in range(foot.shape[0]):
        edge = np.diff(np.concatenate([[0], foot[row].astype(np.int8), [0]]))
        for x0, x1 in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):
            runs.append((row - ky, x0 - kx, x1 - 1 - kx))
    if not 1 <= len(runs) <= MAX_RANK_RUNS:
        raise ValueError("a window of the focal order statistics has 1 .. %d row runs, got %d" % (MAX_RANK_RUNS, len(runs)))
    return np.array(runs, dtype=np.int32)


def _rank_grid(a, name, like):
    """A float32 grid of the DSM's shape, never converted."""
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    if tuple(a.shape) != tuple(like.shape) or a.dtype not in (np.float32, torch.float32):
        raise ValueError("%s is float32 of the DSM's shape %s, got %s %s" % (name, tuple(like.shape), a.dtype, tuple(a.shape)))
    return a


def _focal_select(z, runs, nodata, fr, centre):
    """smvs_dsm_focal_select over the levels fr in chunks of 4 -> n int32 (gh, gw), lo, hi float32 (Q, gh, gw).  A chunk without
    a level between two ranks (num % den == 0 throughout) asks for no hi: it is lo."""
    gh, gw = z.shape
    n = torch.empty((gh, gw), dtype=torch.int32, device=z.device)
    lo = torch.empty((len(fr), gh, gw), dtype=torch.float32, device=z.device)
    hi = torch.empty_like(lo)
    for s0 in range(0, len(fr), MAX_RANK_LEVELS):
        chunk = fr[s0:s0 + MAX_RANK_LEVELS]
        split = any(num % den != 0 for num, den in chunk)
        _call(z.device, "smvs_dsm_focal_select", z, gw, gh, nodata, runs, int(runs.shape[0]), np.array(chunk, dtype=np.int32), len(chunk),
              centre, n if s0 == 0 else None, lo[s0:s0 + len(chunk)], hi[s0:s0 + len(chunk)] if split else None)
        if not split:
            hi[s0:s0 + len(chunk)] = lo[s0:s0 + len(chunk)]
    return n, lo, hi


def _focal_quantiles(z, runs, fr, method, centre, min_valid, nodata):
    n, lo, hi = _focal_select(z, runs, nodata, fr, centre)
    lo_rank, _, rem, den = quantile_ranks(n.reshape(-1), fr)
    grids = lambda t: t.t().reshape(lo.shape)                # (cells, Q) -> (Q, gh, gw)
    value = _quantile_value(lo, hi, grids(lo_rank), grids(rem), den[:, None, None], method)
    value = torch.where((n >= max(min_valid, 1))[None], value, torch.full_like(value, float("nan")))
    return n, lo, hi, value


def focal_quantiles(dsm, window, q=(0.5,), method="linear", centre=None, min_valid=1, nodata=-999.0):
    """Exact quantiles of the heights in every cell's window (include/satmvs.h smvs_dsm_focal_select, DESIGN.md section 9, "Focal
    order statistics"): dsm (gh, gw) float32, never converted; a cell is valid iff finite and != nodata; window as _window_runs()
    takes it, clipped at the grid.  q, method: as in label_quantiles().  With centre ((gh, gw) float32) the statistics at cell p
    are those of |v - centre[p]| (float64 difference, rounded to float32 once); a p whose centre is not finite has no cell.
    -> dict: n_valid int32 (gh, gw), the valid cells of the window; lo, hi float32 (Q, gh, gw), the order statistics of
    quantile_ranks(), input values with their own bits, nodata where n_valid is 0; value float64 (Q, gh, gw) by `method`, NaN
    where n_valid < max(min_valid, 1).  Selection, no sums: equal bits from run to run.  numpy if the DSM came as numpy."""
    dsm = _dsm_bits(dsm)
    runs = _window_runs(window)
    fr = _quantile_fractions(q)
    if method not in QUANTILE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (QUANTILE_METHODS, method))
    if centre is not None:
        centre = _rank_grid(centre, "centre", dsm)
    min_valid = _int_checked(min_valid, "min_valid", 0, 2 ** 31 - 1)
    z, as_numpy = _to_device(dsm)
    c = None if centre is None else _to_device(centre, dev=z.device)[0]
    n, lo, hi, value = _focal_quantiles(z, runs, fr, method, c, min_valid, float(nodata))
    return {k: _back(as_numpy, t) for k, t in (("n_valid", n), ("lo", lo), ("hi", hi), ("value", value))}


def focal_median(dsm, window, min_valid=1, nodata=-999.0, fill=False):
    """The DSM under a median filter of any window within +-32 cells: a valid cell becomes (float) of the "midpoint" median of its
    window's valid cells, despike()'s median: v[n / 2] of the sorted values, or (float)(0.5 ((double)v[n / 2 - 1] +
    (double)v[n / 2])) for even n; nodata where the window holds fewer than max(min_valid, 1) valid cells.  Invalid cells keep
    their bits; with `fill` they are treated like the valid ones.  -> (gh, gw) float32."""
    dsm = _dsm_bits(dsm)
    runs = _window_runs(window)
    min_valid = _int_checked(min_valid, "min_valid", 0, 2 ** 31 - 1)
    z, as_numpy = _to_device(dsm)
    n, _, _, value = _focal_quantiles(z, runs, [(1, 2)], "midpoint", None, min_valid, float(nodata))
    out = _focal_grid(value[0], n >= max(min_valid, 1), nodata)
    return _back(as_numpy, out if fill else torch.where(_valid_cells(z, nodata), out, z))


def _focal_nmad(z, runs, min_valid, nodata):
    n, _, _, median = _focal_quantiles(z, runs, [(1, 2)], "linear", None, min_valid, nodata)
    _, _, _, mad = _focal_quantiles(z, runs, [(1, 2)], "linear", median[0].float(), min_valid, nodata)
    return n, median[0], mad[0]


def focal_nmad(dsm, window, min_valid=1, nodata=-999.0):
    """The robust centre and spread of every cell's window, label_nmad() about a cell: median float64 (gh, gw), the linear median
    of focal_quantiles(); mad, the linear median of |v - float32(median)| over the same window; nmad = 1.4826 mad; n_valid
    int32.  NaN where n_valid < max(min_valid, 1).  -> dict."""
    dsm = _dsm_bits(dsm)
    runs = _window_runs(window)
    min_valid = _int_checked(min_valid, "min_valid", 0, 2 ** 31 - 1)
    z, as_numpy = _to_device(dsm)
    n, median, mad = _focal_nmad(z, runs, min_valid, float(nodata))
    return dict(zip(("median", "mad", "nmad", "n_valid"), _back(as_numpy, median, mad, mad * NMAD_FACTOR, n)))


def despike_robust(dsm, window, k=3.0, floor=0.5, min_valid=3, nodata=-999.0, return_removed=False):
    """despike() beyond its 7 x 7 window and with a threshold the neighbourhood sets itself: a valid cell becomes nodata iff its
    window holds fewer than min_valid valid cells or |(double)z - median| > max(k nmad, floor), median and nmad from
    focal_nmad() (floor [m] keeps flat ground, where nmad is 0, from losing every cell).  Every other cell is copied bit for bit.
    -> the cleaned (gh, gw) float32 (and, with return_removed, a uint8 map of the removed cells)."""
    dsm = _dsm_bits(dsm)
    runs = _window_runs(window)
    k, floor = _finite(k, "k"), _finite(floor, "floor")
    if k < 0.0 or floor < 0.0:
        raise ValueError("k and floor must be >= 0, got %r and %r" % (k, floor))
    min_valid = _int_checked(min_valid, "min_valid", 1, 2 ** 31 - 1)
    z, as_numpy = _to_device(dsm)
    n, median, mad = _focal_nmad(z, runs, min_valid, float(nodata))
    far = (z.double() - median).abs() > torch.clamp(k * (mad * NMAD_FACTOR), min=floor)
    removed = _valid_cells(z, nodata) & ((n < min_valid) | far)
    out = torch.where(removed, torch.full_like(z, float(nodata)), z)
    out, removed = _back(as_numpy, out, removed.to(torch.uint8))
    return (out, removed) if return_removed else out


def _focal_counts(z, runs, t, nodata):
    gh, gw = z.shape
    n, below, equal = (torch.empty((gh, gw), dtype=torch.int32, device=z.device) for _ in range(3))
    _call(z.device, "smvs_dsm_focal_count", z, gw, gh, nodata, runs, int(runs.shape[0]), t, n, below, equal)
    return n, below, equal


def focal_counts(dsm, window, threshold=None, nodata=-999.0):
    """Where a threshold stands among the valid cells of every cell's window (include/satmvs.h smvs_dsm_focal_count): n the
    valid cells, below those under the threshold in the order of the keys (-0.0 below +0.0), equal those with its bits' key;
    int32 (gh, gw) each, below and equal -1 where the threshold is a NaN.  threshold: None = the cell's own height, a number, or
    a (gh, gw) float32 grid (a selected value: below <= rank < below + equal certifies it).  -> (n, below, equal)."""
    dsm = _dsm_bits(dsm)
    runs = _window_runs(window)
    number = isinstance(threshold, (int, float, np.floating, np.integer)) and not isinstance(threshold, bool)
    if threshold is not None and not number:
        threshold = _rank_grid(threshold, "threshold", dsm)
    z, as_numpy = _to_device(dsm)
    t = z if threshold is None else torch.full_like(z, float(threshold)) if number else _to_device(threshold, dev=z.device)[0]
    return _back(as_numpy, *_focal_counts(z, runs, t, float(nodata)))


def elevation_percentile(dsm, window, min_valid=2, nodata=-999.0):
    """The share of a cell's neighbourhood that lies below it, the robust counterpart of tpi() and dev(): at a valid cell whose
    window holds n >= max(min_valid, 2) valid cells, (below + 0.5 (equal - 1)) / (n - 1) with focal_counts() at the cell's own
    height: 0 at the lowest cell of its window, 1 at the highest, ties share the middle of their ranks.  NaN elsewhere.
    -> (gh, gw) float64."""
    dsm = _dsm_bits(dsm)
    runs = _window_runs(window)
    min_valid = _int_checked(min_valid, "min_valid", 0, 2 ** 31 - 1)
    z, as_numpy = _to_device(dsm)
    n, below, equal = _focal_counts(z, runs, z, float(nodata))
    share = (below.double() + 0.5 * (equal.double() - 1.0)) / (n.double() - 1.0)
    keep = _valid_cells(z, nodata) & (n >= max(min_valid, 2))
    return _back(as_numpy, torch.where(keep, share, torch.full_like(share, float("nan"))))


# ---- outlines: a label map as oriented rings of lattice corners, GeoJSON, and rings burnt back into a label map ---------------
MAX_OUTLINE_CELLS = 2 ** 29                                       # 4 edges per cell in an int32


def _label_count_checked(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n < 2 ** 31:
        raise ValueError("n must be an integer in 0 .. 2^31 - 1, got %r" % (n,))
    return int(n)


def _int32_array(a, name, ndim, like):
    """A numpy array or tensor of `like`'s kind, int32 with ndim axes, never converted."""
    if isinstance(a, torch.Tensor) != isinstance(like, torch.Tensor):
        raise ValueError("%s and vertices must both be numpy arrays or both be tensors" % name)
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
    if a.dtype not in (np.int32, torch.int32):
        raise ValueError("%s is int32, got %s" % (name, a.dtype))
    if a.ndim != ndim:
        raise ValueError("%s has %d axes, got shape %s" % (name, ndim, tuple(a.shape)))
    return a


def outlines(labels, n, grid=None):
    """The outlines of the labels 1 .. n of a label map as polygon rings (include/satmvs.h smvs_dsm_outline_count / _write,
    DESIGN.md section 9, "Outlines"): labels (gh, gw) int32 from label(), extract_objects() or changes(), fewer than 2^29 cells;
    values outside 1 .. n count as background.  Corner (x, y) of the lattice is the upper-left corner of cell (row y, col x).
    -> dict: label int32 (n_rings); area2 int64 (n_rings), twice the enclosed area in cells, > 0 for an exterior ring
      (counter-clockwise north up), < 0 for a hole (clockwise); edges int32 (n_rings, 2), unit edges heading E or W and N or S;
      offset int32 (n_rings + 1) into vertices; first_ring int32 (n + 1), the rings of label k + 1 are first_ring[k] ..
      first_ring[k + 1] - 1, the exterior first; vertices int32 (n_vertices, 2) x, y, no collinear points, a ring not closed
      (its last vertex joins its first).  Rings are sorted by (label, start y, start x), a ring starts at its smallest corner.
      with grid (a DSMGrid of the labels' shape): vertices_en float64 (n_vertices, 2) east, north; perimeter_m float64
      (n_rings); label_perimeter_m float64 (n) and n_holes int32 (n) per label.
    Connectivity-8 labels can give a ring that touches itself at a corner; label with connectivity 4 for strictly simple rings.
    Everything depends on labels and n alone, bit for bit.  numpy if the labels came as numpy, device tensors otherwise.  The
    host reads the device's counts twice; for device tensors a damaged workspace shows as offset[-1] == -1 and is not raised."""
    labels = _labels_checked(labels)
    n = _label_count_checked(n)
    gh, gw = int(labels.shape[0]), int(labels.shape[1])
    if gh * gw >= MAX_OUTLINE_CELLS:
        raise ValueError("outlines take fewer than 2^29 cells, got %d x %d" % (gh, gw))
    if grid is not None:
        _on_grid(labels, grid)
    lab, as_numpy = _to_device(labels)
    dev = lab.device
    ne = nr = nv = 0
    ws = nbytes = None
    if n:
        lib = _lib.load()
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        nbytes = lib.smvs_dsm_outline_workspace_bytes(gw, gh, 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _call(dev, "smvs_dsm_outline_count", lab, gw, gh, n, 0, counts, ws, nbytes)
        ne = int(counts[0].item())
        if ne > 0:
            nbytes = lib.smvs_dsm_outline_workspace_bytes(gw, gh, ne)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _call(dev, "smvs_dsm_outline_count", lab, gw, gh, n, ne, counts, ws, nbytes)
            ne, nr, nv = counts.tolist()
        if ne < 0:
            raise _lib.SatMVSNativeError("smvs_dsm_outline_count gave up: an index out of range in its workspace (n_edges = %d)" % ne)
    out = {"label": torch.empty(nr, dtype=torch.int32, device=dev), "area2": torch.empty(nr, dtype=torch.int64, device=dev),
           "edges": torch.empty((nr, 2), dtype=torch.int32, device=dev), "offset": torch.zeros(nr + 1, dtype=torch.int32, device=dev),
           "first_ring": torch.zeros(n + 1, dtype=torch.int32, device=dev), "vertices": torch.empty((nv, 2), dtype=torch.int32, device=dev)}
    if ne:
        _call(dev, "smvs_dsm_outline_write", lab, gw, gh, n, ne, nr, nv, out["label"], out["area2"], out["edges"], out["offset"],
              out["first_ring"], out["vertices"], ws, nbytes)
    if grid is not None:
        xres, yres = float(grid.xres), float(grid.yres)
        v = out["vertices"].double()
        out["vertices_en"] = torch.stack([float(grid.e0) + (v[:, 0] - 0.5) * xres, float(grid.n0) - (v[:, 1] - 0.5) * yres], dim=1)
        out["perimeter_m"] = out["edges"][:, 0].double() * xres + out["edges"][:, 1].double() * yres
        k = out["label"].long() - 1
        per_label = torch.zeros((n, 2), dtype=torch.int64, device=dev).index_add_(0, k, out["edges"].long())       # integer sums
        out["label_perimeter_m"] = per_label[:, 0].double() * xres + per_label[:, 1].double() * yres
        out["n_holes"] = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, k, (out["area2"] < 0).long()).to(torch.int32)
    out = {key: _back(as_numpy, t) for key, t in out.items()}
    if as_numpy and out["offset"][-1] != nv:
        raise _lib.SatMVSNativeError("smvs_dsm_outline_write gave up: an index out of range in its workspace")
    return out


def _rings_checked(vertices, offset, ring_label=None):
    """The ring table of burn_rings, burn_polygons and simplify_outlines, checked on the host as far as it can be without
    reading device memory.  -> vertices, offset, ring_label, n_vertices, n_rings."""
    if not isinstance(vertices, torch.Tensor):
        vertices = np.asarray(vertices)
    vertices = _int32_array(vertices, "vertices", 2, vertices)
    if vertices.shape[1] != 2:
        raise ValueError("vertices are (n_vertices, 2) x, y, got shape %s" % (tuple(vertices.shape),))
    offset = _int32_array(offset, "offset", 1, vertices)
    nv, nr = int(vertices.shape[0]), int(offset.shape[0]) - 1
    if ring_label is not None:
        ring_label = _int32_array(ring_label, "ring_label", 1, vertices)
        nr = int(ring_label.shape[0])
    if int(offset.shape[0]) != nr + 1 or nr < 0:
        raise ValueError("offset has n_rings + 1 = %d entries, got %d" % (nr + 1, int(offset.shape[0])))
    return vertices, offset, ring_label, nv, nr


def _offset_rises(offset, nv):
    if not isinstance(offset, torch.Tensor) and (offset[0] != 0 or offset[-1] != nv or (np.diff(offset) < 0).any()):
        raise ValueError("offset must rise from 0 to n_vertices = %d" % nv)


def _burn(entry, vertices, offset, ring_label, shape):
    """-> (labels on the device, whether the caller gave numpy, the entry's flag bits)."""
    vertices, offset, ring_label, nv, nr = _rings_checked(vertices, offset, ring_label)
    gh, gw = _int_pair(shape, "shape")
    if gh < 1 or gw < 1 or gh * gw >= 2 ** 31:
        raise ValueError("shape has positive sizes and fewer than 2^31 cells, got %d x %d" % (gh, gw))
    _offset_rises(offset, nv)
    v, as_numpy = _to_device(vertices)
    dev = v.device
    off, _ = _to_device(offset, dev=dev)
    lab, _ = _to_device(ring_label, dev=dev)
    out = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _call(dev, entry, v, off, lab, nr, nv, gw, gh, out, flag)
    bits = int(flag.item())
    if bits & 2:
        raise ValueError("offset must rise from 0 to n_vertices = %d" % nv)
    return out, as_numpy, bits


def burn_rings(vertices, offset, ring_label, shape):
    """Rings burnt into a label map, the reverse of outlines() (include/satmvs.h smvs_dsm_burn): vertices (n_vertices, 2) int32
    x, y on the lattice of outlines(), offset (n_rings + 1) int32 into them, ring_label (n_rings) int32, shape = (gh, gw).
    Every vertical ring edge toggles its label along its rows and every row takes its running XOR: the even-odd rule at cell
    centres, so a hole empties what its exterior ring fills and a ring given twice cancels.  Rings may lie partly or wholly off
    the grid.  Edges run along the lattice: one whose ends differ in both coordinates is a ValueError.
    burn_rings(r["vertices"], r["offset"], r["label"], labels.shape) of r = outlines(labels, n) is labels with the values outside
    1 .. n zeroed.  -> labels (gh, gw) int32; numpy if the vertices came as numpy, a device tensor otherwise."""
    out, as_numpy, bits = _burn("smvs_dsm_burn", vertices, offset, ring_label, shape)
    if bits & 1:
        raise ValueError("a ring edge whose ends differ in both coordinates: burn_rings takes edges along the lattice only")
    return _back(as_numpy, out)


MAX_POLYGON_COORD = 2 ** 20                                       # |x|, |y| below it: the crossing's numerator fits an int64


def burn_polygons(vertices, offset, ring_label, shape):
    """burn_rings for rings with edges of any direction (include/satmvs.h smvs_dsm_burn_polygons): the rings of
    simplify_outlines(), or any polygons with integer vertices |x|, |y| < 2^20, on or off the grid.  A cell belongs to a ring
    iff its centre is inside by the even-odd rule; a centre exactly on an edge belongs to the side on the edge's left (the cell
    counts as right of the crossing only if its centre lies strictly right of it), so a centre on the border two polygons share
    is in exactly one of them.  On rings with lattice edges the result is burn_rings' bit for bit.
    -> labels (gh, gw) int32; numpy if the vertices came as numpy, a device tensor otherwise."""
    out, as_numpy, bits = _burn("smvs_dsm_burn_polygons", vertices, offset, ring_label, shape)
    if bits & 4:
        raise ValueError("a vertex outside |x|, |y| < 2^20")
    return _back(as_numpy, out)


MAX_SIMPLIFY_COORD = 32767                                        # with it every product of the distance key stays below 2^63
MAX_TOL16 = 65535
SIMPLIFY_BATCH = 8                                                # rounds between two reads of the device's status


def _tol16_checked(tol):
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not math.isfinite(tol) or tol < 0:
        raise ValueError("tol is a finite number of cells >= 0, got %r" % (tol,))
    tol16 = int(math.floor(16.0 * float(tol)))
    if tol16 > MAX_TOL16:
        raise ValueError("tol must be below 4096 cells (floor(16 tol) <= %d), got %r" % (MAX_TOL16, tol))
    return tol16


def simplify_outlines(rings, tol, grid=None):
    """The rings of outlines() simplified by Douglas-Peucker in exact integers (include/satmvs.h, "Simplified outlines"; DESIGN.md
    section 9): rings is the dict of outlines(), or any dict with vertices (n_vertices, 2) int32 0 <= x, y <= 32767, offset
    (n_rings + 1) int32, label (n_rings) int32 and first_ring; tol in cells, used as tol16 = floor(16 tol) <= 65535.
    Every ring keeps its first vertex and the vertex farthest from it; a segment between two kept vertices splits at its
    farthest vertex (distance to the segment; ties to the vertex nearest the segment's middle, then the lower index) iff that
    distance is strictly above tol16 / 16, so the whole ring as given lies within tol of the result.  A ring left with fewer than
    3 vertices, no area or an area of the other sign keeps all its vertices (simplified 0).  Nothing else is repaired: a large
    tol can make rings cross themselves or each other, and a border shared by two labels is simplified once from each side.
    -> dict: label, first_ring as given; offset int32 (n_rings + 1); vertices int32 (n_vertices_out, 2); area2 int64 (n_rings),
      the shoelace sum of the ring as returned; kept int32 (n_vertices_out), the index of every output vertex in the input
      vertices; simplified uint8 (n_rings); rounds int, the number of rounds up to and with the first in which no segment split
      (0 without vertices).  with grid: vertices_en float64 (n_vertices_out, 2), perimeter_m float64 (n_rings), the sum of
      sqrt((dx xres)^2 + (dy yres)^2) over the ring's edges, and n_holes int32 per label.
    tol 0 returns every ring of outlines() unchanged.  Everything depends on the input alone, bit for bit.  numpy if the
    vertices came as numpy, device tensors otherwise; write_geojson() and burn_polygons() take the result."""
    for key in ("vertices", "offset", "label", "first_ring"):
        if key not in rings:
            raise ValueError("rings is the dict of outlines(): entry %r is missing" % key)
    vertices, offset, label, nv, nr = _rings_checked(rings["vertices"], rings["offset"], rings["label"])
    first_ring = _int32_array(rings["first_ring"], "first_ring", 1, vertices)
    tol16 = _tol16_checked(tol)
    _offset_rises(offset, nv)
    if nv and not isinstance(vertices, torch.Tensor) and (vertices.min() < 0 or vertices.max() > MAX_SIMPLIFY_COORD):
        raise ValueError("vertices must be in 0 .. %d" % MAX_SIMPLIFY_COORD)
    if grid is not None:
        _grid_checked(grid, "grid")
    v, as_numpy = _to_device(vertices)
    dev = v.device
    off, _ = _to_device(offset, dev=dev)
    lab, _ = _to_device(label, dev=dev)
    first, _ = _to_device(first_ring, dev=dev)
    lib = _lib.load()
    nbytes = lib.smvs_dsm_simplify_workspace_bytes(nr, nv)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    word = torch.empty(2, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_simplify_begin", v, off, nr, nv, word, ws, nbytes)
    bits = int(word[0].item())
    if bits & 2:
        raise ValueError("offset must rise from 0 to n_vertices = %d" % nv)
    if bits & 1:
        raise ValueError("vertices must be in 0 .. %d" % MAX_SIMPLIFY_COORD)
    rounds = 0
    if nv:
        longest = int((off[1:] - off[:-1]).max().item())             # a ring of m vertices splits in at most m rounds
        run = 0
        while True:
            _call(dev, "smvs_dsm_simplify_rounds", v, off, nr, nv, tol16, SIMPLIFY_BATCH, word, ws, nbytes)
            run += SIMPLIFY_BATCH
            splits, rounds = word.tolist()
            if splits < 0:
                raise _lib.SatMVSNativeError("smvs_dsm_simplify_rounds gave up: an index out of range in its workspace")
            if splits == 0:
                break
            if run > longest:
                raise _lib.SatMVSNativeError("smvs_dsm_simplify_rounds: segments still split after %d rounds, more than the longest ring has vertices (%d)" % (run, longest))
    _call(dev, "smvs_dsm_simplify_count", v, off, nr, nv, word, ws, nbytes)
    n_out = int(word[0].item())
    if n_out < 0:
        raise _lib.SatMVSNativeError("smvs_dsm_simplify_count gave up: an index out of range in its workspace")
    out = {"label": lab, "first_ring": first, "offset": torch.zeros(nr + 1, dtype=torch.int32, device=dev),
           "vertices": torch.empty((n_out, 2), dtype=torch.int32, device=dev), "area2": torch.empty(nr, dtype=torch.int64, device=dev),
           "kept": torch.empty(n_out, dtype=torch.int32, device=dev), "simplified": torch.empty(nr, dtype=torch.uint8, device=dev)}
    _call(dev, "smvs_dsm_simplify_write", v, off, nr, nv, n_out, out["offset"], out["vertices"], out["area2"], out["kept"], out["simplified"], ws, nbytes)
    if grid is not None:
        xres, yres = float(grid.xres), float(grid.yres)
        p = out["vertices"].double()
        out["vertices_en"] = torch.stack([float(grid.e0) + (p[:, 0] - 0.5) * xres, float(grid.n0) - (p[:, 1] - 0.5) * yres], dim=1)
        o = out["offset"].long()
        ring_of = torch.repeat_interleave(torch.arange(nr, device=dev), o[1:] - o[:-1], output_size=n_out)
        at = torch.arange(n_out, device=dev)
        nxt = torch.where(at + 1 == o[1:][ring_of], o[:-1][ring_of], at + 1)             # the ring's last vertex joins its first
        d = p[nxt] - p
        length = torch.sqrt((d[:, 0] * xres) ** 2 + (d[:, 1] * yres) ** 2)
        # a ring's lengths added one after the other in vertex order: no atomics, so equal bits from run to run
        out["perimeter_m"] = torch.segment_reduce(length, "sum", lengths=o[1:] - o[:-1], unsafe=True) if nr else length.new_zeros(0)
        n = int(first.numel()) - 1
        k = lab.long() - 1
        inside = (k >= 0) & (k < n)
        out["n_holes"] = torch.zeros(max(n, 0), dtype=torch.int64, device=dev).index_add_(0, k[inside], (out["area2"] < 0).long()[inside]).to(torch.int32)
    if as_numpy:
        torch.cuda.synchronize(dev)
    result = {key: _back(as_numpy, t) for key, t in out.items()}
    if int(result["offset"][-1]) != n_out:
        raise _lib.SatMVSNativeError("smvs_dsm_simplify_write gave up: an index out of range in its workspace")
    result["rounds"] = int(rounds)
    return result


def _json_value(x):
    """A property of a feature: numpy scalars and arrays as what the json module writes; a float that is not finite as null."""
    if isinstance(x, np.ndarray):
        return [_json_value(e) for e in x]
    if isinstance(x, (np.bool_, bool)):
        return bool(x)
    if isinstance(x, (np.integer, int)):
        return int(x)
    x = float(x)
    return x if math.isfinite(x) else None


def write_geojson(path, rings, grid, stats=None, projection=None):
    """The rings of outlines() as a GeoJSON FeatureCollection (RFC 7946 winding: exterior rings counter-clockwise, holes
    clockwise): one Feature per label that has a ring, a Polygon with the label's exterior ring first and then its holes, every
    ring closed by repeating its first vertex.  Coordinates are east, north on `grid`; with `projection` (a
    TransverseMercator) lon, lat through its EastNorth2latlon.  properties: label, and from `stats` (the dict of label_stats,
    extract_objects or changes, entry k for label k + 1) every 1-D entry as a scalar and every 2-D entry (bbox, centroid) as a
    list.  A label map in which one label has several components gives a Polygon with several counter-clockwise rings, which
    is not valid GeoJSON: label first.  Plain json, no GIS library.  -> the number of features."""
    host = {k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for k, t in rings.items()}
    label, offset, first, v = host["label"], host["offset"], host["first_ring"], host["vertices"]
    n = len(first) - 1
    if v.ndim != 2 or v.shape[1] != 2 or len(offset) != len(label) + 1 or (len(label) and first[-1] != len(label)):
        raise ValueError("rings is the dict of outlines()")
    _grid_checked(grid, "grid")
    table = {}
    for key, t in (stats or {}).items():
        t = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        if t.ndim not in (1, 2) or t.shape[0] != n:
            raise ValueError("stats[%r] has shape %s: one entry per label (%d) expected" % (key, tuple(t.shape), n))
        table[key] = t
    en = np.stack([float(grid.e0) + (v[:, 0].astype(np.float64) - 0.5) * float(grid.xres),
                   float(grid.n0) - (v[:, 1].astype(np.float64) - 0.5) * float(grid.yres)], axis=1)
    if projection is not None and len(en):
        en = np.asarray(projection.EastNorth2latlon(en))[:, ::-1]
    features = []
    for k in range(n):
        if first[k] == first[k + 1]:
            continue
        polygon = []
        for r in range(first[k], first[k + 1]):
            ring = en[offset[r]:offset[r + 1]].tolist()
            polygon.append(ring + ring[:1])
        properties = {"label": k + 1}
        properties.update({key: _json_value(t[k]) for key, t in table.items()})
        features.append({"type": "Feature", "properties": properties, "geometry": {"type": "Polygon", "coordinates": polygon}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)
        f.write("\n")
    return len(features)


# ---- contour lines ---------------------------------------------------------------------------------------------------------------
MAX_CONTOUR_LEVELS = 4096                                         # levels of one native call; more go in chunks
MAX_CONTOUR_Z = 32768.0
MAX_CONTOUR_LIST = 2 ** 20                                        # levels of one contours() call


def _contour_dsm(dsm, grid=None):
    """A (gh, gw) DSM of any real dtype, numpy taken as float32 (a tensor is converted on its way to the device), fewer than
    2^29 cells; checked before any device work."""
    if not isinstance(dsm, torch.Tensor):
        dsm = np.asarray(dsm, dtype=np.float32)
    if dsm.ndim != 2:
        raise ValueError("a DSM is (gh, gw), got shape %s" % (tuple(dsm.shape),))
    gh, gw = int(dsm.shape[0]), int(dsm.shape[1])
    if gh < 1 or gw < 1 or gh * gw >= MAX_OUTLINE_CELLS:
        raise ValueError("contours take positive sizes and fewer than 2^29 cells, got %d x %d" % (gh, gw))
    if grid is not None:
        _on_grid(dsm, _grid_checked(grid, "grid"))
    return dsm


def _interval_checked(interval, base):
    if isinstance(interval, bool) or not isinstance(interval, (int, float, np.integer, np.floating)) or not math.isfinite(interval) or interval <= 0:
        raise ValueError("interval is a finite number of metres > 0, got %r" % (interval,))
    return float(interval), _finite(base, "base")


def contour_levels(dsm, interval, base=0.0, nodata=-999.0):
    """The levels base + k interval, k an integer, that lie strictly inside the range of the DSM's valid heights (finite,
    != nodata, |z| <= 32768 m) -> float64 numpy, rising; empty without two different valid heights.  numpy stays on the host."""
    interval, base = _interval_checked(interval, base)
    dsm = _contour_dsm(dsm)
    if isinstance(dsm, torch.Tensor):
        z = dsm.to(torch.float32)
        z = z[torch.isfinite(z) & (z != float(np.float32(nodata))) & (z.abs() <= MAX_CONTOUR_Z)]
        if z.numel() == 0:
            return np.zeros(0, np.float64)
        lo, hi = float(z.min().item()), float(z.max().item())
    else:
        with np.errstate(invalid="ignore"):
            z = dsm[np.isfinite(dsm) & (dsm != np.float32(nodata)) & (np.abs(dsm) <= np.float32(MAX_CONTOUR_Z))]
        if z.size == 0:
            return np.zeros(0, np.float64)
        lo, hi = float(z.min()), float(z.max())
    k0, k1 = math.floor((lo - base) / interval), math.ceil((hi - base) / interval)
    if k1 - k0 + 1 > MAX_CONTOUR_LIST:
        raise ValueError("interval %r gives more than 2^20 levels between %r and %r" % (interval, lo, hi))
    levels = base + np.arange(k0, k1 + 1, dtype=np.float64) * interval
    return levels[(levels > lo) & (levels < hi)]


def _level_keys(levels):
    """Levels in metres -> the odd int64 K = 2 floor(256 level) + 1 in units of 2^-9 m, rising."""
    lv = np.asarray(levels.cpu() if isinstance(levels, torch.Tensor) else levels, dtype=np.float64)
    if lv.ndim != 1:
        raise ValueError("levels is a list of heights in metres, got shape %s" % (tuple(lv.shape),))
    if lv.size > MAX_CONTOUR_LIST:
        raise ValueError("at most 2^20 levels in a call, got %d" % lv.size)
    if not np.isfinite(lv).all():
        raise ValueError("levels must be finite")
    if lv.size and np.abs(lv).max() > MAX_CONTOUR_Z:
        raise ValueError("levels must lie within +-32768 m")
    keys = np.sort(2 * np.floor(256.0 * lv).astype(np.int64) + 1)
    if (np.diff(keys) == 0).any():
        raise ValueError("two levels fall on the same step of 2^-8 m (levels are used as 2 floor(256 level) + 1 half steps)")
    return keys


def _contour_chunk(z, gw, gh, nodata, keys, want_edge=True):
    """One native pass over at most 4096 levels -> the device tensors of smvs_dsm_contour_write and n_vertices."""
    dev = z.device
    lib = _lib.load()
    n = len(keys)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    nbytes = lib.smvs_dsm_contour_workspace_bytes(gw, gh, n, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _call(dev, "smvs_dsm_contour_count", z, gw, gh, nodata, keys, n, 0, counts, ws, nbytes)
    nc, nl, nv = int(counts[0].item()), 0, 0
    if nc > 0:
        nbytes = lib.smvs_dsm_contour_workspace_bytes(gw, gh, n, nc)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _call(dev, "smvs_dsm_contour_count", z, gw, gh, nodata, keys, n, nc, counts, ws, nbytes)
        nc, nl, nv = counts.tolist()
    if nc < 0:
        raise _lib.SatMVSNativeError("smvs_dsm_contour_count gave up: more than 2^31 - 1 crossings, or an index out of range in its workspace")
    out = {"level_index": torch.empty(nl, dtype=torch.int32, device=dev), "closed": torch.empty(nl, dtype=torch.uint8, device=dev),
           "offset": torch.zeros(nl + 1, dtype=torch.int32, device=dev), "first_line": torch.zeros(n + 1, dtype=torch.int32, device=dev),
           "vertices": torch.empty((nv, 2), dtype=torch.float64, device=dev), "edge": torch.empty(nv, dtype=torch.int32, device=dev)}
    if nl:
        _call(dev, "smvs_dsm_contour_write", z, gw, gh, nodata, keys, n, nc, nl, nv, out["level_index"], out["closed"], out["offset"],
              out["first_line"], out["vertices"], out["edge"] if want_edge else None, ws, nbytes)
    return out, nv


def contours(dsm, levels=None, interval=None, base=0.0, grid=None, nodata=-999.0):
    """The contour lines of a DSM (include/satmvs.h smvs_dsm_contour_count / _write, DESIGN.md section 9, "Contours"): dsm
    (gh, gw) of any real dtype (taken as float32), fewer than 2^29 cells; exactly one of levels [m, any order, used sorted] and
    interval [m; the levels of contour_levels(dsm, interval, base)].  Heights count in steps of 2^-8 m and a level as
    K = 2 floor(256 level) + 1 half steps: at most 2^-8 m above what was asked, never on a node.  A vertex lies on a lattice edge
    between two cell centres, x = column, y = row in index units; a line keeps the higher ground on its left, north up (a ring
    round a hill runs counter-clockwise); lines end at voids and at the grid's edge and are not joined across them.
    -> dict: level_index int32 (n_lines) into the sorted levels; level float64 (n_lines), the effective level K / 512;
      closed bool (n_lines), a closed line's first vertex is not repeated; offset int32 (n_lines + 1) into vertices; first_line
      int32 (n_levels + 1), the lines of level k are first_line[k] .. first_line[k + 1] - 1; vertices float64 (n_vertices, 2)
      x, y; edge int32 (n_vertices), the lattice edge 2 (row gw + col) + (0 east, 1 south) of every vertex.  Lines are sorted by
      (level, edge of the first vertex); an open line starts where it enters, a ring at its smallest edge.
      with grid (a DSMGrid of the DSM's shape): vertices_en float64 (n_vertices, 2) east, north (cell centres, no half-cell
      shift) and length_m float64 (n_lines), a ring's closing segment included.
    More than 4096 levels go through several native calls and give the result of one.  Everything depends on dsm, nodata and
    the levels alone, bit for bit.  numpy if the DSM came as numpy, device tensors otherwise.  The host reads the device's
    counts twice per native pass; for device tensors a damaged workspace shows as offset[-1] == -1 and is not raised."""
    if (levels is None) == (interval is None):
        raise ValueError("give exactly one of levels and interval")
    dsm = _contour_dsm(dsm, grid)
    if interval is not None:
        levels = contour_levels(dsm, interval, base, nodata)
    keys = _level_keys(levels)
    z, as_numpy = _to_device(dsm, torch.float32)
    dev = z.device
    gh, gw = z.shape
    parts, total, n_lines = [], 0, 0
    for k0 in range(0, len(keys), MAX_CONTOUR_LEVELS):
        part, nv = _contour_chunk(z, gw, gh, float(nodata), np.ascontiguousarray(keys[k0:k0 + MAX_CONTOUR_LEVELS], np.int32))
        if parts:                                            # what one call over all the levels would have given
            part["level_index"] += k0
            part["offset"] = part["offset"][1:] + total
            part["first_line"] = part["first_line"][1:] + n_lines
        parts.append(part)
        total += nv
        n_lines += int(part["level_index"].numel())
    if parts:
        out = {key: torch.cat([p[key] for p in parts]) for key in parts[0]}
    else:
        out = {"level_index": torch.empty(0, dtype=torch.int32, device=dev), "closed": torch.empty(0, dtype=torch.uint8, device=dev),
               "offset": torch.zeros(1, dtype=torch.int32, device=dev), "first_line": torch.zeros(1, dtype=torch.int32, device=dev),
               "vertices": torch.empty((0, 2), dtype=torch.float64, device=dev), "edge": torch.empty(0, dtype=torch.int32, device=dev)}
    out["closed"] = out["closed"].bool()
    out["level"] = torch.from_numpy(keys.astype(np.float64) / 512.0).to(dev)[out["level_index"].long()]
    if grid is not None:
        nl = int(out["level_index"].numel())
        v, o = out["vertices"], out["offset"].long()
        en = torch.stack([float(grid.e0) + v[:, 0] * float(grid.xres), float(grid.n0) - v[:, 1] * float(grid.yres)], dim=1)
        out["vertices_en"] = en
        line_of = torch.repeat_interleave(torch.arange(nl, device=dev), o[1:] - o[:-1], output_size=total)
        at = torch.arange(total, device=dev)
        last = at + 1 == o[1:][line_of]
        d = en[torch.where(last, o[:-1][line_of], at + 1)] - en                       # a line's last vertex joins its first ...
        length = torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
        length = torch.where(last & ~out["closed"][line_of], torch.zeros_like(length), length)      # ... if the line is closed
        # a line's lengths added one after the other in vertex order: no atomics, so equal bits from run to run
        out["length_m"] = torch.segment_reduce(length, "sum", lengths=o[1:] - o[:-1], unsafe=True) if nl else length.new_zeros(0)
    out = {key: _back(as_numpy, t) for key, t in out.items()}
    if as_numpy and int(out["offset"][-1]) != total:
        raise _lib.SatMVSNativeError("smvs_dsm_contour_write gave up: an index out of range in its workspace")
    return out


def write_contours(path, lines, grid, projection=None):
    """The lines of contours() as a GeoJSON FeatureCollection of LineStrings, one Feature per line in the lines' order; a closed
    line repeats its first vertex.  Coordinates are east, north on `grid` (E = e0 + x xres, N = n0 - y yres); with `projection`
    (a TransverseMercator) lon, lat through its EastNorth2latlon.  properties: level_m (the effective level), closed, length_m
    (on the grid, in metres, a ring's closing segment included).  Plain json, no GIS library.  -> the number of features."""
    host = {k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for k, t in lines.items()}
    for key in ("level", "closed", "offset", "vertices"):
        if key not in host:
            raise ValueError("lines is the dict of contours(): entry %r is missing" % key)
    level, closed, offset, v = host["level"], host["closed"], host["offset"], host["vertices"]
    if v.ndim != 2 or v.shape[1] != 2 or len(offset) != len(level) + 1 or len(closed) != len(level) or int(offset[-1]) != len(v):
        raise ValueError("lines is the dict of contours()")
    _grid_checked(grid, "grid")
    en = np.stack([float(grid.e0) + v[:, 0].astype(np.float64) * float(grid.xres),
                   float(grid.n0) - v[:, 1].astype(np.float64) * float(grid.yres)], axis=1)
    out = en
    if projection is not None and len(en):
        out = np.asarray(projection.EastNorth2latlon(en))[:, ::-1]
    features = []
    for i in range(len(level)):
        a, b = int(offset[i]), int(offset[i + 1])
        ends = [a] if closed[i] else []
        if "length_m" in host:
            length = host["length_m"][i]
        else:
            p = en[list(range(a, b)) + ends]
            length = 0.0
            for s in np.sqrt(((p[1:] - p[:-1]) ** 2).sum(axis=1)):
                length += float(s)
        properties = {"level_m": _json_value(level[i]), "closed": bool(closed[i]), "length_m": _json_value(length)}
        features.append({"type": "Feature", "properties": properties,
                         "geometry": {"type": "LineString", "coordinates": out[list(range(a, b)) + ends].tolist()}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)
        f.write("\n")
    return len(features)


# ---- hydrology: depression filling, D8 directions, accumulation, basins ---------------------------------------------------------
MAX_HYDRO_CELLS = 2 ** 30                                         # the Euler tour's 2 gw gh elements in an int32
FLOOD_BATCH = 8                                                   # rounds of the first batch; one read of the device's status per batch
MAX_FLOOD_BATCH = 4096                                            # smvs_dsm_flood_rounds takes no more
FLOW_ENCODINGS = ("index", "esri")


def _hydro_dsm(dsm, grid=None):
    """A (gh, gw) float32 DSM, never converted (filling gives untouched cells back bit for bit), fewer than 2^30 cells."""
    dsm = _dsm_bits(dsm)
    if int(dsm.shape[0]) * int(dsm.shape[1]) >= MAX_HYDRO_CELLS:
        raise ValueError("hydrology takes fewer than 2^30 cells, got %d x %d" % (int(dsm.shape[0]), int(dsm.shape[1])))
    if grid is not None:
        _on_grid(dsm, _grid_checked(grid, "grid"))
    return dsm


def _flood(z, nodata, batch=None):
    """The flood keys of a device DSM -> (keys (gh, gw) int64 holding the uint64 words, rounds run)."""
    dev = z.device
    gh, gw = z.shape
    nbytes = _lib.load().smvs_dsm_flood_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keys = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_flood_begin", z, gw, gh, nodata, keys, ws, nbytes)

    def rounds(step):
        _call(dev, "smvs_dsm_flood_rounds", z, gw, gh, nodata, keys, step, status, ws, nbytes)
        return int(status.item())
    return keys, _relax(rounds, gw * gh, "smvs_dsm_flood_rounds", batch)


def _relax(rounds, cells, name, batch=None):
    """The batch loop of the tile relaxations (flood, cost distance): rounds(k) runs k global rounds and returns the device's
    status, read once; 8 rounds, then doubling (batch=k fixes it), until a batch ends with no tile changed -> the rounds run.
    More than cells + 2 rounds cannot be: SatMVSNativeError."""
    run, step, grow = 0, batch or FLOOD_BATCH, batch is None
    while True:
        status = rounds(step)
        run += step
        if status == 0:
            return run
        if run > cells + 2:
            raise _lib.SatMVSNativeError("%s: tiles still change after %d rounds, more than the grid has cells (%d)" % (name, run, cells))
        if grow:
            step = min(2 * step, MAX_FLOOD_BATCH)


def fill_depressions(dsm, nodata=-999.0, return_depth=False, return_rounds=False, batch=None):
    """A DTM without pits (include/satmvs.h, "Hydrology"): dsm (gh, gw) float32, never converted, fewer
    than 2^30 cells; valid = finite, != nodata and |z| <= 32768 m.  Heights count in steps of 2^-8 m; water leaves at the grid's
    edge and into voids; the result is the lowest surface >= the input from which every cell drains, 8-connected.  A cell the
    fill does not raise comes back with its own bits, a raised one as a multiple of 2^-8 m; invalid cells come back as nodata.
    -> filled (gh, gw) float32; with return_depth also depth (gh, gw) float32 = filled - input, exact, >= 0 (nodata where
    invalid) and flat_dist (gh, gw) int32, the steps to the flat's way out (0 where a strictly lower neighbour or an outlet is,
    -1 where invalid); with return_rounds also the global rounds run, a multiple of the batches.  The host reads the device's
    status once per batch of rounds (8, then doubling; batch=k fixes it).  numpy if the DSM came as numpy, tensors otherwise."""
    dsm = _hydro_dsm(dsm)
    if batch is not None:
        batch = _int_checked(batch, "batch", 1, MAX_FLOOD_BATCH)
    z, as_numpy = _to_device(dsm)
    gh, gw = z.shape
    keys, rounds = _flood(z, float(nodata), batch)
    filled = torch.empty_like(z)
    depth = torch.empty_like(z) if return_depth else None
    flat = torch.empty((gh, gw), dtype=torch.int32, device=z.device) if return_depth else None
    _call(z.device, "smvs_dsm_flood_read", z, gw, gh, float(nodata), keys, filled, depth, flat)
    out = (filled,) + ((depth, flat) if return_depth else ())
    out = _back(as_numpy, *out)
    if not return_rounds:
        return out
    return (out if isinstance(out, tuple) else (out,)) + (rounds,)


def flow_codes(encoding="index"):
    """The uint8 table that turns the library's direction codes into `encoding`: entry c is the code written for c.  "index":
    the codes as they are (0 outlet, k + 1 towards neighbour k = E, SE, S, SW, W, NW, N, NE, 255 invalid).  "esri": 1, 2, 4, ...,
    128 for E, SE, ..., NE, 0 for an outlet, 255 for invalid (ArcGIS Hydrology's numbers)."""
    if encoding not in FLOW_ENCODINGS:
        raise ValueError("encoding must be one of %s, got %r" % (FLOW_ENCODINGS, encoding))
    table = np.full(256, 255, np.uint8)
    table[:9] = np.arange(9) if encoding == "index" else [0] + [1 << k for k in range(8)]
    return table


def flow_distances(grid):
    """The eight step lengths E, SE, S, SW, W, NW, N, NE on `grid` [m], float64: xres, yres and np.hypot(xres, yres)."""
    _grid_checked(grid, "grid")
    x, y = float(grid.xres), float(grid.yres)
    h = float(np.hypot(x, y))
    return np.array([x, h, y, h, x, h, y, h], np.float64)


def flow_direction(dsm, grid, nodata=-999.0, encoding="index"):
    """D8 directions of a DSM (include/satmvs.h, "Hydrology"): the flood of fill_depressions(), then every cell's receiver:
    the neighbour down the steepest slope of the FILLED surface, (w_c - w_n) / distance as one float64 division with the
    distances of flow_distances(grid), ties to the lowest k; on a flat the neighbour one step nearer the flat's way out.  The
    directions form a forest rooted at the outlets: no cycles, no pits.
    -> (gh, gw) uint8 in `encoding` (flow_codes()): "index" 0 outlet, k + 1, 255 invalid; "esri" 1, 2, 4, ..., 128.
    flow_accumulation() and basins() take the "index" codes.  numpy if the DSM came as numpy, a device tensor otherwise."""
    dsm = _hydro_dsm(dsm, grid)
    table = flow_codes(encoding)
    dist = flow_distances(grid)
    z, as_numpy = _to_device(dsm)
    gh, gw = z.shape
    keys, _ = _flood(z, float(nodata))
    codes = torch.empty((gh, gw), dtype=torch.uint8, device=z.device)
    _call(z.device, "smvs_dsm_flow_dir", keys, gw, gh, dist, codes)
    if encoding != "index":
        codes = torch.from_numpy(table).to(z.device)[codes.long()]
    return _back(as_numpy, codes)


def _codes_checked(direction):
    if not isinstance(direction, torch.Tensor):
        direction = np.asarray(direction)
    if direction.ndim != 2:
        raise ValueError("directions are (gh, gw), got shape %s" % (tuple(direction.shape),))
    if direction.dtype not in (np.uint8, torch.uint8):
        raise ValueError("directions are uint8 codes (flow_codes('index')), got %s" % (direction.dtype,))
    gh, gw = int(direction.shape[0]), int(direction.shape[1])
    if gh < 1 or gw < 1 or gh * gw >= MAX_HYDRO_CELLS:
        raise ValueError("directions have positive sizes and fewer than 2^30 cells, got %d x %d" % (gh, gw))
    return direction


def _flow_workspace(d):
    gh, gw = d.shape
    nbytes = _lib.load().smvs_dsm_flow_workspace_bytes(gw, gh)
    if nbytes == 0:
        raise ValueError("unsupported direction grid: %d x %d cells" % (gw, gh))
    return torch.empty(nbytes, dtype=torch.uint8, device=d.device), nbytes


def flow_accumulation(direction, weights=None, grid=None, cycles="raise"):
    """Flow accumulation over a direction grid (include/satmvs.h, "Hydrology"): direction (gh, gw) uint8 "index" codes, from
    flow_direction() or edited; codes 9 .. 254 count as 255; a code whose target is off the grid or invalid makes a root.
    Every cell gets the sum of `weights` ((gh, gw) int32, never converted; None: 1 per cell) over itself and everything
    upstream; invalid cells get 0.  A cell on a cycle, or draining into one, has no sum: ValueError, or with cycles="mark" the
    value -1 in every such cell.  -> (gh, gw) int64 [cells, or units of the weights]; with grid (a DSMGrid of that shape)
    float64 [m^2] = cells xres yres (and -1 stays -1).  Exact integer sums by an Euler tour of the flow forest: the number of
    launches follows log(gw gh), not the longest river.  numpy if the directions came as numpy, a device tensor otherwise."""
    direction = _codes_checked(direction)
    if cycles not in ("raise", "mark"):
        raise ValueError("cycles must be 'raise' or 'mark', got %r" % (cycles,))
    if weights is not None:
        if not isinstance(weights, torch.Tensor):
            weights = np.asarray(weights)
        if weights.dtype not in (np.int32, torch.int32) or tuple(weights.shape) != tuple(direction.shape):
            raise ValueError("weights are int32 of the directions' shape, got %s %s" % (weights.dtype, tuple(weights.shape)))
    if grid is not None:
        _on_grid(direction, _grid_checked(grid, "grid"))
    d, as_numpy = _to_device(direction)
    dev = d.device
    w = None if weights is None else _to_device(weights, dev=dev)[0]
    gh, gw = d.shape
    ws, nbytes = _flow_workspace(d)
    acc = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_flow_accumulate", d, w, gw, gh, acc, flag, ws, nbytes)
    cyclic = bool(int(flag.item()) & 1)
    if cyclic and cycles == "raise":
        raise ValueError("the directions hold a cycle: some cells reach no root; cycles='mark' gives them -1")
    if grid is not None:
        area = acc.double() * (float(grid.xres) * float(grid.yres))
        acc = torch.where(_cyclic_cells(d, ws, nbytes), torch.full_like(area, -1.0), area) if cyclic else area
    return _back(as_numpy, acc)


def _cyclic_cells(d, ws, nbytes):
    """The cells of a device direction grid without a root, as the basins see them (valid, and labelled 0 without pour points)."""
    gh, gw = d.shape
    basin = torch.empty((gh, gw), dtype=torch.int32, device=d.device)
    word = torch.empty(2, dtype=torch.int32, device=d.device)
    _call(d.device, "smvs_dsm_flow_basins", d, None, gw, gh, basin, word[:1], word[1:], ws, nbytes)
    return (d <= 8) & (basin == 0)


def _pour_checked(pour_points, shape):
    """(whether it is a mask, the mask or the (m, 2) list), checked before any device work."""
    gh, gw = shape
    p = pour_points if isinstance(pour_points, torch.Tensor) else np.asarray(pour_points)
    if tuple(p.shape) == (gh, gw):
        return True, _mask_checked(p)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("pour_points is a (gh, gw) mask or an (m, 2) list of (row, col), got shape %s" % (tuple(p.shape),))
    integral = not (p.is_floating_point() or p.is_complex() or p.dtype == torch.bool) if isinstance(p, torch.Tensor) else np.issubdtype(p.dtype, np.integer)
    if not integral:
        raise ValueError("pour points (row, col) are integers, got %s" % (p.dtype,))
    if p.shape[0] and (int(p.min()) < 0 or int(p[:, 0].max()) >= gh or int(p[:, 1].max()) >= gw):
        raise ValueError("pour points must lie on the %d x %d grid" % (gh, gw))
    return False, p


def _pour_mask(is_mask, p, shape, dev):
    if is_mask:
        if not isinstance(p, torch.Tensor):
            p = np.not_equal(p, 0).view(np.uint8)
        return (_to_device(p, dev=dev)[0] != 0).to(torch.uint8).contiguous()
    rc = torch.as_tensor(p).to(dev).long()
    mask = torch.zeros(shape, dtype=torch.uint8, device=dev)
    mask[rc[:, 0], rc[:, 1]] = 1
    return mask


def basins(direction, pour_points=None):
    """Catchments of a direction grid (include/satmvs.h, "Hydrology"): every cell gets the number of the root it drains to,
    the roots numbered 1 .. n in row-major order; invalid cells and cells on or into a cycle get 0.  With pour_points, a
    (gh, gw) mask (bool or integer, non-zero = pour point) or an (m, 2) integer list of (row, col): the pour cells are cut from
    their receivers and are the only numbered roots, so a pour point upstream of another splits its river, and everything that
    passes no pour point is 0; a pour point on an invalid cell counts for nothing.  A (2, 2) grid takes a (2, 2) array as a mask.
    -> (labels (gh, gw) int32, n); label_stats(), outlines() and write_geojson() take them.  numpy if the directions came as
    numpy, a device tensor otherwise.  Reading n is the one synchronisation."""
    direction = _codes_checked(direction)
    pour = None if pour_points is None else _pour_checked(pour_points, tuple(direction.shape))
    d, as_numpy = _to_device(direction)
    dev = d.device
    gh, gw = d.shape
    if pour is not None:
        pour = _pour_mask(*pour, (gh, gw), dev)
    ws, nbytes = _flow_workspace(d)
    basin = torch.empty((gh, gw), dtype=torch.int32, device=dev)
    word = torch.empty(2, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_flow_basins", d, pour, gw, gh, basin, word[:1], word[1:], ws, nbytes)
    return _back(as_numpy, basin), int(word[0].item())


def streams(acc, threshold):
    """The cells whose accumulation reaches `threshold` (in the units of acc: cells, or m^2 with a grid) -> bool mask; torch
    or numpy as acc comes."""
    threshold = _finite(threshold, "threshold")
    if not isinstance(acc, torch.Tensor):
        acc = np.asarray(acc)
    if acc.ndim != 2:
        raise ValueError("acc is (gh, gw), got shape %s" % (tuple(acc.shape),))
    return acc >= threshold


def depressions(dsm, grid, min_depth=0.5, min_area_m2=50.0, nodata=-999.0):
    """The depressions of a DSM as objects: fill_depressions(return_depth=True); foreground = depth >= float32(min_depth);
    label() (8-connected); label_stats(values=depth, grid=grid); sieve_labels() at ceil(min_area_m2 / (xres yres)) cells, as
    extract_objects() is built.  In a satellite DTM most are noise and filled voids, which makes depth a quality product.
    -> (labels (gh, gw) int32, stats: label_stats' dict of the depressions that stay, max = the greatest depth, volume = the
    water they hold [m^3], depth (gh, gw) float32).  The table goes straight into outlines() / write_geojson().  numpy if the
    DSM came as numpy, device tensors otherwise."""
    dsm = _hydro_dsm(dsm, grid)
    min_depth, min_area_m2 = float(min_depth), float(min_area_m2)
    if not (math.isfinite(min_depth) and min_depth > 0.0):
        raise ValueError("min_depth must be finite and > 0, got %r" % min_depth)
    if not (math.isfinite(min_area_m2) and min_area_m2 >= 0.0):
        raise ValueError("min_area_m2 must be finite and >= 0, got %r" % min_area_m2)
    min_cells = _int_checked(int(math.ceil(min_area_m2 / (float(grid.xres) * float(grid.yres)))), "min_area_m2 in cells", 0, 2 ** 31 - 1)
    z, as_numpy = _to_device(dsm)
    _, depth, _ = fill_depressions(z, nodata, return_depth=True)
    fg = torch.isfinite(depth) & (depth != float(np.float32(nodata))) & (depth >= float(np.float32(min_depth)))
    labels, n = label(fg, 8)
    stats = label_stats(labels, n, values=depth, grid=grid, nodata=nodata)
    labels, _, kept = sieve_labels(labels, stats["area"], min_cells)
    stats = {k: t[kept] for k, t in stats.items()}
    return _back(as_numpy, labels), {k: _back(as_numpy, t) for k, t in stats.items()}, _back(as_numpy, depth)


# ---- stream network: Strahler orders, links as polylines, flow length -----------------------------------------------------------
STREAM_KEYS = ("order_map", "link", "head", "order", "next_link", "offset", "vertices", "steps")


def _cycles_checked(cycles):
    if cycles not in ("raise", "mark"):
        raise ValueError("cycles must be 'raise' or 'mark', got %r" % (cycles,))
    return cycles


def _stream_inputs(direction, stream, cycles, grid=None):
    """(codes, mask as uint8 0 / 1, as_numpy), both on the directions' device, everything checked before any device work."""
    direction = _codes_checked(direction)
    _cycles_checked(cycles)
    stream = _mask_checked(stream)
    if tuple(stream.shape) != tuple(direction.shape):
        raise ValueError("stream mask shape %s differs from the directions' %s" % (tuple(stream.shape), tuple(direction.shape)))
    if grid is not None:
        _on_grid(direction, _grid_checked(grid, "grid"))
    if not isinstance(stream, torch.Tensor):
        stream = np.not_equal(stream, 0).view(np.uint8)
    d, as_numpy = _to_device(direction)
    m = (_to_device(stream, dev=d.device)[0] != 0).to(torch.uint8).contiguous()
    return d, m, as_numpy


def _stream_workspace(d):
    gh, gw = d.shape
    nbytes = _lib.load().smvs_dsm_stream_workspace_bytes(gw, gh)
    if nbytes == 0:
        raise ValueError("unsupported direction grid: %d x %d cells" % (gw, gh))
    return torch.empty(nbytes, dtype=torch.uint8, device=d.device), nbytes


def _stream_order(d, m, ws, nbytes, cycles, want_link=True):
    """smvs_dsm_stream_order on device tensors -> order map, link map (or None), the four counts read once."""
    dev = d.device
    gh, gw = d.shape
    order = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    link = torch.empty((gh, gw), dtype=torch.int32, device=dev) if want_link else None
    word = torch.empty(5, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_stream_order", d, m, gw, gh, order, link, word[:4], word[4:], ws, nbytes)
    word = [int(x) for x in word.tolist()]
    if word[4] & 1 and cycles == "raise":
        raise ValueError("the directions hold a cycle: some cells reach no root; cycles='mark' leaves them out of the network")
    return order, link, word[:4]


def _steps_length(steps, grid):
    """(n_ew xres + n_ns yres) + n_diag hypot(xres, yres), float64, one rounding per operation in exactly that order."""
    s = steps.double()
    return (s[..., 0] * float(grid.xres) + s[..., 1] * float(grid.yres)) + s[..., 2] * float(np.hypot(float(grid.xres), float(grid.yres)))


def stream_order(direction, stream, cycles="raise"):
    """Strahler orders of a stream mask over a direction grid (include/satmvs.h, "Stream network"):
    direction (gh, gw) uint8 "index" codes as flow_accumulation() takes them; stream (gh, gw), bool or any integer dtype,
    non-zero = a stream cell, from streams() or any mask at all.  The stream cells are the masked cells that reach a root; a
    cell flows into its receiver if that is a stream cell too, so a gap in the mask cuts the network and nothing upstream of it
    counts below.  A cell without inflow has order 1; otherwise, with m the greatest order flowing in, m + 1 if two inflows
    have it and m if one.  A cell on a cycle, or draining into one, is no stream cell: ValueError if the grid holds one (masked
    or not), unless cycles="mark".  -> (gh, gw) uint8, 0 outside the network.  The number of launches follows log(gw gh), not
    the longest river.  numpy if the directions came as numpy, a device tensor otherwise."""
    d, m, as_numpy = _stream_inputs(direction, stream, cycles)
    ws, nbytes = _stream_workspace(d)
    order, _, _ = _stream_order(d, m, ws, nbytes, cycles, want_link=False)
    return _back(as_numpy, order)


def stream_links(direction, stream, grid=None, cycles="raise"):
    """The stream network as links (include/satmvs.h, "Stream network"): inputs and orders as stream_order().  A stream cell is
    a head iff the number of stream cells flowing into it is not 1 (a source or a junction); every head starts one link, which
    runs downstream until the next cell is a junction or there is none (a mouth).  Links are numbered 0 .. n - 1 in row-major
    order of their heads.  -> dict:
      order_map uint8 (gh, gw); link int32 (gh, gw), link number + 1 on the network and 0 elsewhere: label_stats() takes it
      head int32 (n), the head's cell index row gw + col; order int32 (n); next_link int32 (n), the link the last cell flows
        into, -1 at a mouth; offset int32 (n + 1) into vertices
      vertices int32 (n_vertices, 2) col, row: a link's cells, head first, then the junction it flows into, so that lines
        connect; a link of one cell at a mouth has one vertex
      steps int32 (n, 3): the E-W, N-S and diagonal segments of the polyline
      with grid (a DSMGrid of the directions' shape): vertices_en float64 (n_vertices, 2) east, north at cell centres and
        length_m float64 (n) = (n_ew xres + n_ns yres) + n_diag hypot(xres, yres), exact in its integers.
    Everything depends on the two inputs alone, bit for bit.  numpy if the directions came as numpy, device tensors otherwise.
    The host reads the device's counts once between the two native passes."""
    d, m, as_numpy = _stream_inputs(direction, stream, cycles, grid)
    dev = d.device
    gh, gw = d.shape
    ws, nbytes = _stream_workspace(d)
    order_map, link, (_, nl, nv, _) = _stream_order(d, m, ws, nbytes, cycles)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)                # noqa: E731
    out = {"order_map": order_map, "link": link, "head": i32(nl), "order": i32(nl), "next_link": i32(nl), "offset": torch.zeros(nl + 1, dtype=torch.int32, device=dev),
           "vertices": i32(nv, 2), "steps": i32(nl, 3)}
    if nl:
        _call(dev, "smvs_dsm_stream_write", d, m, gw, gh, nl, nv, out["head"], out["order"], out["next_link"], out["offset"], out["vertices"],
              out["steps"], ws, nbytes)
        if int(out["offset"][nl].item()) != nv:
            raise _lib.SatMVSNativeError("smvs_dsm_stream_write: the network's counts differ from n_links = %d, n_vertices = %d" % (nl, nv))
    if grid is not None:
        v = out["vertices"].double()
        out["vertices_en"] = torch.stack([float(grid.e0) + v[:, 0] * float(grid.xres), float(grid.n0) - v[:, 1] * float(grid.yres)], dim=1)
        out["length_m"] = _steps_length(out["steps"], grid)
    return {k: _back(as_numpy, t) for k, t in out.items()}


def flow_length(direction, grid=None, cycles="raise"):
    """The length of every cell's flow path to its root (include/satmvs.h, "Stream network"): direction as flow_accumulation()
    takes it.  -> int32 (gh, gw, 3), the E-W, N-S and diagonal steps of the path; a root has (0, 0, 0); invalid cells get -1, and
    so do cells on or into a cycle under cycles="mark" (ValueError otherwise).  With grid (a DSMGrid of that shape): float64
    (gh, gw) metres = (n_ew xres + n_ns yres) + n_diag hypot(xres, yres), NaN at invalid cells and -1 at cyclic ones.  The
    counts are exact; the number of launches follows log(gw gh).  numpy if the directions came as numpy, a device tensor
    otherwise."""
    direction = _codes_checked(direction)
    _cycles_checked(cycles)
    if grid is not None:
        _on_grid(direction, _grid_checked(grid, "grid"))
    d, as_numpy = _to_device(direction)
    dev = d.device
    gh, gw = d.shape
    ws, nbytes = _stream_workspace(d)
    steps = torch.empty((gh, gw, 3), dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_flow_length", d, gw, gh, steps, flag, ws, nbytes)
    if int(flag.item()) & 1 and cycles == "raise":
        raise ValueError("the directions hold a cycle: some cells reach no root; cycles='mark' gives them -1")
    if grid is None:
        return _back(as_numpy, steps)
    metres = _steps_length(steps, grid)
    metres = torch.where(steps[..., 0] < 0, torch.full_like(metres, -1.0), metres)
    return _back(as_numpy, torch.where(d > 8, torch.full_like(metres, float("nan")), metres))


def write_streams(path, links, grid, projection=None):
    """The links of stream_links() as a GeoJSON FeatureCollection of LineStrings, one Feature per link of two vertices or more
    in the links' order (a link of one cell at a mouth has no line).  Coordinates are east, north at cell centres on `grid`
    (E = e0 + col xres, N = n0 - row yres); with `projection` (a TransverseMercator) lon, lat through its EastNorth2latlon.
    properties: link (its number), order (Strahler), next_link (-1 at a mouth), n_cells (the link's own cells, the junction it
    ends in not counted) and length_m = (n_ew xres + n_ns yres) + n_diag hypot(xres, yres).  Plain json, no GIS library.
    -> the number of features."""
    host = {k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for k, t in links.items()}
    for key in ("order", "next_link", "offset", "vertices", "steps"):
        if key not in host:
            raise ValueError("links is the dict of stream_links(): entry %r is missing" % key)
    order, nxt, offset, v, steps = host["order"], host["next_link"], host["offset"], host["vertices"], host["steps"]
    n = len(order)
    if v.ndim != 2 or v.shape[1] != 2 or len(offset) != n + 1 or len(nxt) != n or tuple(steps.shape) != (n, 3) or int(offset[-1]) != len(v):
        raise ValueError("links is the dict of stream_links()")
    _grid_checked(grid, "grid")
    en = np.stack([float(grid.e0) + v[:, 0].astype(np.float64) * float(grid.xres),
                   float(grid.n0) - v[:, 1].astype(np.float64) * float(grid.yres)], axis=1)
    out = en
    if projection is not None and len(en):
        out = np.asarray(projection.EastNorth2latlon(en))[:, ::-1]
    s = steps.astype(np.float64)
    length = (s[:, 0] * float(grid.xres) + s[:, 1] * float(grid.yres)) + s[:, 2] * float(np.hypot(float(grid.xres), float(grid.yres)))
    features = []
    for i in range(n):
        a, b = int(offset[i]), int(offset[i + 1])
        if b - a < 2:
            continue
        properties = {"link": i, "order": int(order[i]), "next_link": int(nxt[i]), "n_cells": b - a - (1 if nxt[i] >= 0 else 0),
                      "length_m": _json_value(length[i])}
        features.append({"type": "Feature", "properties": properties, "geometry": {"type": "LineString", "coordinates": out[a:b].tolist()}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)
        f.write("\n")
    return len(features)


def extract_streams(dtm, grid, min_area_m2=25000.0, nodata=-999.0):
    """The drainage network of a DTM: flow_direction(dtm, grid) -> flow_accumulation(grid=grid) -> streams(acc, min_area_m2) ->
    stream_links(grid=grid).  min_area_m2 is the catchment a channel needs before it counts as one; the default (1000 cells of
    5 m) is a choice for 5 m grids, not tuned on real data.  -> the dict of stream_links() with vertices_en and length_m.
    numpy if the DTM came as numpy, device tensors otherwise."""
    dtm = _hydro_dsm(dtm, grid)
    min_area_m2 = float(min_area_m2)
    if not (math.isfinite(min_area_m2) and min_area_m2 >= 0.0):
        raise ValueError("min_area_m2 must be finite and >= 0, got %r" % min_area_m2)
    z, as_numpy = _to_device(dtm)
    code = flow_direction(z, grid, nodata)
    acc = flow_accumulation(code, grid=grid)
    links = stream_links(code, streams(acc, min_area_m2), grid=grid)
    return {k: _back(as_numpy, t) for k, t in links.items()}


# ---- cost distance: accumulated cost, back-links as a D8 forest, least-cost paths -----------------------------------------------
MAX_COST_CELLS = 2 ** 24                                          # w < 2^38 and fewer steps than cells keep D below 2^62
MAX_COST_LENGTH = 32767                                           # a step length in units of 2^-8 m
MAX_COST_FACTOR = 65535                                           # a friction or a table entry in units of 2^-8
COST_UNIT = 32768.0                                               # D counts 2^-15 cost metre
NO_MAX_COST = 2 ** 64 - 1


def cost_terms(grid):
    """The eight step lengths of cost_distance() on `grid`, int32 in units of 2^-8 m: rint(256 flow_distances(grid)[k]) for
    k = E, SE, S, SW, W, NW, N, NE.  ValueError if one leaves 1 .. 32767 (cells below 2^-8 m, or a diagonal above 127 m)."""
    L = np.rint(256.0 * flow_distances(grid))
    if not (np.isfinite(L).all() and L.min() >= 1 and L.max() <= MAX_COST_LENGTH):
        raise ValueError("the step lengths of the grid must lie in 2^-8 m .. 127.99 m, got %s m" % (flow_distances(grid).tolist(),))
    return L.astype(np.int32)


def slope_table(fn):
    """The vertical factor of cost_distance() as its int32[256] table: bin b holds the steps with floor(32 tan(slope)) = b - 128
    (the two end bins take everything beyond -4 and +4); fn, a Python callable of tan(slope), is evaluated at the bin centres
    (b - 127.5) / 32 and stored as rint(256 value).  A value that is not finite or is <= 0 gives 0, which forbids the step (so
    does a positive value below 1 / 512); a value above 65535 / 256 is a ValueError.  Floats on the host only: the device
    sees the integers."""
    table = np.zeros(256, np.int32)
    for b in range(256):
        v = float(fn((b - 127.5) / 32.0))
        if not math.isfinite(v) or v <= 0.0:
            continue
        if v > MAX_COST_FACTOR / 256.0:
            raise ValueError("the vertical factor at tan(slope) = %g is %g, above 65535 / 256" % ((b - 127.5) / 32.0, v))
        table[b] = int(np.rint(256.0 * v))
    return table


def tobler_table():
    """slope_table() of walking: the pace relative to level ground from Tobler's hiking function, v = 6 exp(-3.5 |tan + 0.05|)
    km/h, so exp(3.5 (|tan + 0.05| - 0.05)), times the surface length of the step, sqrt(1 + tan^2) = 1 / cos(slope).  Where the
    product passes 65535 / 256 (beyond about 56 degrees either way) the step is forbidden.  tan is the rise in the direction of
    travel: cost_distance() reads it towards the sources, and away from them with reverse=True."""
    def factor(t):
        v = math.exp(3.5 * (abs(t + 0.05) - 0.05)) * math.sqrt(1.0 + t * t)
        return v if v <= MAX_COST_FACTOR / 256.0 else float("nan")
    return slope_table(factor)


def quantise_friction(friction, nodata=-999.0):
    """A float friction grid [cost per metre] as the uint16 grid cost_distance() takes: rint(256 f) computed in float64, 0 (a
    barrier) where f is not finite, equals nodata (compared in the grid's own dtype) or is <= 0.  A value above 65535 / 256 is
    a ValueError; a positive one below 1 / 512 becomes a barrier.  numpy in, numpy out; a tensor stays on its device."""
    as_numpy = not isinstance(friction, torch.Tensor)
    f = torch.from_numpy(np.ascontiguousarray(friction)) if as_numpy else friction
    if f.ndim != 2 or not f.is_floating_point():
        raise ValueError("a friction grid is (gh, gw) of a float dtype, got %s %s" % (f.dtype, tuple(f.shape)))
    bad = ~torch.isfinite(f) | (f == torch.tensor(float(nodata), dtype=f.dtype).item()) | (f <= 0)
    q = torch.where(bad, torch.zeros((), dtype=torch.float64, device=f.device), torch.round(256.0 * f.double()))
    if q.numel() and float(q.max()) > MAX_COST_FACTOR:
        raise ValueError("friction above 65535 / 256 = %g does not fit: rescale the grid (got %g)" % (MAX_COST_FACTOR / 256.0, float(q.max()) / 256.0))
    q = q.to(torch.int32).to(torch.uint16)
    return q.numpy() if as_numpy else q


def _friction_checked(friction, shape):
    if not isinstance(friction, torch.Tensor):
        friction = np.asarray(friction)
    if friction.dtype not in (np.uint16, torch.uint16) or tuple(friction.shape) != tuple(shape):
        raise ValueError("friction is uint16 of shape %s in units of 2^-8 (quantise_friction() makes it), got %s %s"
                         % (tuple(shape), friction.dtype, tuple(friction.shape)))
    return friction


def _table_checked(vertical):
    table = np.ascontiguousarray(vertical)
    if table.shape != (256,) or not np.issubdtype(table.dtype, np.integer) or table.min() < 0 or table.max() > MAX_COST_FACTOR:
        raise ValueError("vertical is the int table of slope_table(): 256 entries in 0 .. 65535")
    return table.astype(np.int32)


def _max_cost_units(max_cost):
    """max_cost [cost metre] in the units of D: floor(32768 max_cost); None or +inf: no limit."""
    if max_cost is None:
        return NO_MAX_COST
    max_cost = float(max_cost)
    if math.isnan(max_cost) or max_cost < 0.0:
        raise ValueError("max_cost must be >= 0, got %r" % max_cost)
    return NO_MAX_COST if max_cost * COST_UNIT >= 2.0 ** 63 else int(math.floor(max_cost * COST_UNIT))


def _cost_relax(dev, f, z, gw, gh, nodata, L, table, reverse, keys, ws, nbytes, batch=None):
    """The rounds of cost_distance() on begun keys -> the global rounds run."""
    status = torch.empty(1, dtype=torch.int32, device=dev)

    def rounds(step):
        _call(dev, "smvs_dsm_cost_rounds", f, z, gw, gh, nodata, L, table, reverse, keys, step, status, ws, nbytes)
        return int(status.item())
    return _relax(rounds, gw * gh, "smvs_dsm_cost_rounds", batch)


def cost_distance(sources, grid, friction=None, dsm=None, vertical=None, reverse=False, max_cost=None, nodata=-999.0,
                  return_raw=False, return_rounds=False, batch=None):
    """Cost distance over a grid (include/satmvs.h, "Cost distance"): the accumulated cost of the cheapest
    8-connected trip from every cell to a source, in integers.
      sources   a (gh, gw) mask (bool or integer, non-zero = a source) or an (m, 2) integer list of (row, col), with the rules of
                basins()' pour points; a source on a barrier is no source; no passable source at all is a ValueError
      grid      a DSMGrid of that shape: the step lengths are cost_terms(grid)
      friction  (gh, gw) uint16 from quantise_friction(): cost per metre in units of 2^-8, 0 = a barrier; None = 1.0 everywhere
      dsm, vertical  a (gh, gw) float32 DSM, never converted, and the table of slope_table() / tobler_table(); both or neither.
                Cells without a height (not finite, nodata, |z| > 32768) are barriers; a step c -> n towards the sources costs
                table[bin of (q_n - q_c) / length] in place of 256, and 0 forbids it.  reverse=True reads the slope the other
                way: travel away from the sources
    A step between the neighbours c and n costs w = max(1, (f_c + f_n) L[k] T >> 10) units of 2^-15 cost metre, that is the
    mean friction times the length times the vertical factor; D = 0 at the sources and min(D_n + w) elsewhere.
    -> (cost, backlink): cost float64 (gh, gw) = D / 32768, +Inf where no source is reached, NaN on barriers; backlink uint8 in
    the codes of flow_direction() ("index"): 0 at a source, k + 1 towards the neighbour the cheapest trip goes to (ties to the
    lowest k), 255 at barriers and unreachable cells.  It is a flow forest rooted at the sources: cost_allocation(),
    flow_length(), flow_accumulation() and least_cost_paths() take it as it is.  With max_cost [cost metre] cells with
    D > floor(32768 max_cost) read as unreachable.  With return_raw also D as int64 (-1 at barriers and unreachable cells), with
    return_rounds also the global rounds run.  The host reads the device's status once per batch of rounds (8, then doubling;
    batch=k fixes it).  Every bit depends on the inputs alone.  numpy if the sources came as numpy, device tensors otherwise."""
    _grid_checked(grid, "grid")
    gh, gw = int(grid.height), int(grid.width)
    if gh * gw > MAX_COST_CELLS:
        raise ValueError("cost distance takes at most 2^24 cells, got %d x %d" % (gh, gw))
    L = cost_terms(grid)
    src = _pour_checked(sources, (gh, gw))
    if friction is not None:
        friction = _friction_checked(friction, (gh, gw))
    if (dsm is None) != (vertical is None):
        raise ValueError("dsm and vertical go together: a DSM needs the table of slope_table(), and the table a DSM")
    table = None
    if dsm is not None:
        dsm = _on_grid(_dsm_bits(dsm), grid)
        table = _table_checked(vertical)
    units = _max_cost_units(max_cost)
    if batch is not None:
        batch = _int_checked(batch, "batch", 1, MAX_FLOOD_BATCH)
    as_numpy = not isinstance(sources, torch.Tensor)
    given = [t for t in (sources, friction, dsm) if isinstance(t, torch.Tensor) and t.is_cuda]
    dev = given[0].device if given else _dev()
    s = _pour_mask(*src, (gh, gw), dev)
    f = None if friction is None else _to_device(friction, dev=dev)[0]
    z = None if dsm is None else _to_device(dsm, dev=dev)[0]
    nodata, reverse = float(nodata), int(bool(reverse))
    nbytes = _lib.load().smvs_dsm_cost_workspace_bytes(gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keys = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_cost_begin", f, s, z, gw, gh, nodata, keys, count, ws, nbytes)
    if int(count.item()) == 0:
        raise ValueError("no passable source: every source lies on a barrier, or there is none")
    rounds = _cost_relax(dev, f, z, gw, gh, nodata, L, table, reverse, keys, ws, nbytes, batch)
    cost = torch.empty((gh, gw), dtype=torch.float64, device=dev)
    backlink = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    raw = torch.empty((gh, gw), dtype=torch.int64, device=dev) if return_raw else None
    _call(dev, "smvs_dsm_cost_read", f, z, gw, gh, nodata, L, table, reverse, keys, ctypes.c_ulonglong(units), raw, cost, backlink, ws, nbytes)
    out = _back(as_numpy, *((cost, backlink) + ((raw,) if return_raw else ())))
    return out + (rounds,) if return_rounds else out


def cost_allocation(backlink):
    """The cost allocation of cost_distance(): which source serves each cell.  It is basins(backlink), nothing else: the
    back-links are a direction grid whose roots are the sources, so a cell's basin is the source its cheapest trip ends at.
    The sources are numbered 1 .. n in row-major order of their cells (a source on a barrier has no number); barriers and
    unreachable cells get 0.  -> (labels (gh, gw) int32, n), as basins()."""
    return basins(backlink)


def least_cost_paths(backlink, targets, grid=None, raw=None):
    """The least-cost paths from a set of targets to their sources as a connected network: the forest tools on the back-links
    of cost_distance(), no kernel of their own.  targets: a (gh, gw) mask or an (m, 2) integer list of (row, col), with the
    rules of basins()' pour points.  A target on a barrier or an unreachable cell (back-link 255) is reported, not followed.
    The corridor is flow_accumulation(backlink, weights=targets) > 0, every cell some target's path passes, and the result is
    stream_links(backlink, corridor, grid): paths that meet merge into one link from there on, and a link's `order` is the
    Strahler order of the merged network.  -> that dict, which write_streams() takes as it is, and per target, in the order of
    the list (row-major for a mask):
      target_cell int32 (m, 2) row, col; target_link int32 (m), the link the target lies on (following next_link from it
        leads to the source), -1 for a target that is not followed
      target_steps int32 (m, 3), the E-W, N-S and diagonal steps of its path (flow_length(); -1 where not followed), and with
        grid target_length_m float64 (m) = (n_ew xres + n_ns yres) + n_diag hypot(xres, yres), NaN where not followed
      with raw (cost_distance(return_raw=True)) target_cost float64 (m) = raw / 32768, +Inf where raw is -1.
    numpy if the back-links came as numpy, device tensors otherwise."""
    backlink = _codes_checked(backlink)
    shape = tuple(int(v) for v in backlink.shape)
    is_mask, p = _pour_checked(targets, shape)
    if grid is not None:
        _on_grid(backlink, _grid_checked(grid, "grid"))
    if raw is not None:
        if not isinstance(raw, torch.Tensor):
            raw = np.asarray(raw)
        if raw.dtype not in (np.int64, torch.int64) or tuple(raw.shape) != shape:
            raise ValueError("raw is int64 of the back-links' shape, got %s %s" % (raw.dtype, tuple(raw.shape)))
    d, as_numpy = _to_device(backlink)
    dev = d.device
    mask = _pour_mask(is_mask, p, shape, dev)
    rc = torch.nonzero(mask) if is_mask else torch.as_tensor(p).to(dev).long().reshape(-1, 2)
    followed = (mask != 0) & (d <= 8)
    acc = flow_accumulation(d, weights=followed.to(torch.int32))
    out = stream_links(d, acc > 0, grid=grid)
    r, c = rc[:, 0], rc[:, 1]
    on = followed[r, c]
    out["target_cell"] = rc.to(torch.int32)
    out["target_link"] = torch.where(on, out["link"][r, c] - 1, torch.full_like(out["link"][r, c], -1))
    steps = flow_length(d)[r, c]
    out["target_steps"] = steps
    if grid is not None:
        out["target_length_m"] = torch.where(on, _steps_length(steps, grid), torch.full((), float("nan"), dtype=torch.float64, device=dev))
    if raw is not None:
        at = _to_device(raw, dev=dev)[0][r, c]
        out["target_cost"] = torch.where(at < 0, torch.full((), float("inf"), dtype=torch.float64, device=dev), at.double() / COST_UNIT)
    return {k: _back(as_numpy, t) for k, t in out.items()}


# ---- seeded flood: geodesic reconstruction, h-maxima, peaks by prominence, the marker watershed ------------------------------------
RECONSTRUCT_METHODS = {"dilation": -1, "erosion": 1}              # the polarity of smvs_dsm_seed_*
MAX_SEED_OFFSET = 2 ** 25                                         # |offset| of smvs_dsm_seed_begin, in quanta of 2^-8 m
MAX_H_QUANTA = 2 ** 24                                            # floor(256 h) of h_maxima(), h_minima(), peaks()


def _domain_checked(mask, shape):
    """A mask of the flood's domain (None: every cell), checked before any device work."""
    if mask is None:
        return None
    mask = _mask_checked(mask)
    if tuple(mask.shape) != tuple(shape):
        raise ValueError("mask shape %s differs from the DSM's %s" % (tuple(mask.shape), tuple(shape)))
    return mask


def _domain(mask, dev):
    """A checked mask -> uint8 on dev (None stays None)."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor):
        mask = np.not_equal(mask, 0).view(np.uint8)
    return (_to_device(mask, dev=dev)[0] != 0).to(torch.uint8).contiguous()


def _h_quanta(h):
    """floor(256 h) of a prominence [m], 1 .. 2^24."""
    h = _finite(h, "h")
    quanta = int(math.floor(h * 256.0))
    if not 1 <= quanta <= MAX_H_QUANTA:
        raise ValueError("floor(256 h) must be in 1 .. 2^24 (h from 2^-8 m to 65536 m), got h = %r" % h)
    return quanta


def _seed_flood(z, marker, domain, nodata, polarity, offset, batch=None, surface=False, steps=False, link=False):
    """The seeded flood of device grids (include/satmvs.h, "Seeded flood") -> dict: the outputs asked for, and "rounds"."""
    dev = z.device
    gh, gw = z.shape
    nbytes = _lib.load().smvs_dsm_seed_workspace_bytes(gw, gh)
    if nbytes == 0:
        raise ValueError("unsupported flood: %d x %d cells" % (gw, gh))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    keys = torch.empty((gh, gw), dtype=torch.int64, device=dev)
    word = torch.empty(2, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_seed_begin", z, marker, domain, gw, gh, nodata, polarity, offset, keys, word[:1], ws, nbytes)

    def rounds(step):
        _call(dev, "smvs_dsm_seed_rounds", z, gw, gh, nodata, polarity, keys, step, word[1:], ws, nbytes)
        return int(word[1].item())
    out = {"rounds": _relax(rounds, gw * gh, "smvs_dsm_seed_rounds", batch)}
    out["surface"] = torch.empty_like(z) if surface else None
    out["steps"] = torch.empty((gh, gw), dtype=torch.int32, device=dev) if steps else None
    out["link"] = torch.empty((gh, gw), dtype=torch.uint8, device=dev) if link else None
    _call(dev, "smvs_dsm_seed_read", z, marker, domain, gw, gh, nodata, polarity, offset, keys, out["surface"], out["steps"], out["link"], None, ws, nbytes)
    return out


def _reconstruct(marker, surface, polarity, offset, mask, nodata, return_steps, return_link, return_rounds, batch):
    surface = _hydro_dsm(surface)
    marker = _dsm_bits(marker)
    if tuple(marker.shape) != tuple(surface.shape):
        raise ValueError("marker shape %s differs from the surface's %s" % (tuple(marker.shape), tuple(surface.shape)))
    mask = _domain_checked(mask, surface.shape)
    if batch is not None:
        batch = _int_checked(batch, "batch", 1, MAX_FLOOD_BATCH)
    z, as_numpy = _to_device(surface)
    m = z if marker is surface else _to_device(marker, dev=z.device)[0]
    got = _seed_flood(z, m, _domain(mask, z.device), float(nodata), polarity, offset, batch, True, return_steps, return_link)
    out = (got["surface"],) + ((got["steps"],) if return_steps else ()) + ((got["link"],) if return_link else ())
    out = _back(as_numpy, *out)
    if not return_rounds:
        return out
    return (out if isinstance(out, tuple) else (out,)) + (got["rounds"],)


def reconstruct(marker, surface, method="dilation", mask=None, nodata=-999.0, return_steps=False, return_link=False, return_rounds=False,
                batch=None):
    """Grey-scale geodesic reconstruction (include/satmvs.h, "Seeded flood") of `marker` under
    (method="dilation") or over ("erosion") `surface`: both (gh, gw) float32, never converted, fewer than 2^30 cells; valid =
    finite, != nodata, |z| <= 32768 m, and inside `mask` (bool or integer, non-zero = inside) when one is given.  Heights count
    in steps of 2^-8 m.  The marker is clamped to the surface (from below for the dilation, from above for the erosion); a valid
    cell with a valid marker is a seed, and the result at a cell is the best level a path from any seed reaches it at: for the
    dilation the highest min(marker at the seed, lowest surface along the path), 8-connected; invalid cells are walls.  A cell
    whose result is the surface comes back with the surface's own bits, every other one as a multiple of 2^-8 m; invalid cells
    and cells no seed reaches (a component without a valid marker) come back as nodata.
    -> the reconstruction (gh, gw) float32; with return_steps also steps (gh, gw) int32, the steps within the flat from where
    the level was set (-1 where nodata); with return_link also the back-links (gh, gw) uint8 in the codes of flow_direction()
    ("index"): 0 at a root (a seed nothing undercut), k + 1 towards the neighbour the flood came from, 255 where nodata: a
    forest that basins(), flow_length() and flow_accumulation() take; with return_rounds also the global rounds run.  The host
    reads the device's status once per batch of rounds (8, then doubling; batch=k fixes it).  Every bit depends on the inputs
    alone.  numpy if the surface came as numpy, device tensors otherwise."""
    if method not in RECONSTRUCT_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(RECONSTRUCT_METHODS), method))
    return _reconstruct(marker, surface, RECONSTRUCT_METHODS[method], 0, mask, nodata, return_steps, return_link, return_rounds, batch)


def h_maxima(dsm, h, mask=None, nodata=-999.0, return_rounds=False, batch=None):
    """The h-maxima transform: the reconstruction by dilation of dsm - h under dsm, which cuts every dome down to what stands
    less than h above its saddle.  One reconstruction with the DSM as its own marker and the offset floor(256 h) quanta (1 ..
    2^24) added on the device in integers: no float32 subtraction is formed on the host.  The other arguments and the result
    as reconstruct()."""
    return _reconstruct(dsm, dsm, -1, _h_quanta(h), mask, nodata, False, False, return_rounds, batch)


def h_minima(dsm, h, mask=None, nodata=-999.0, return_rounds=False, batch=None):
    """The h-minima transform: the reconstruction by erosion of dsm + h over dsm, which fills every pit up to h above its
    floor.  As h_maxima(), with the other polarity."""
    return _reconstruct(dsm, dsm, 1, _h_quanta(h), mask, nodata, False, False, return_rounds, batch)


def _first_cells(lab, n):
    """The first cell in raster order of the labels 1 .. n of a device label map -> int64 (n) flat indices (gh gw where absent)."""
    cells = lab.numel()
    first = torch.full((n + 1,), cells, dtype=torch.int64, device=lab.device)
    flat = lab.reshape(-1).long().clamp(min=0, max=n)
    first.scatter_reduce_(0, flat, torch.arange(cells, device=lab.device), "amin")
    return first[1:]


def peaks(dsm, h, grid=None, mask=None, min_height=None, connectivity=8, nodata=-999.0):
    """The peaks of a DSM by prominence: the cells where q - q(h_maxima(dsm, h)) == floor(256 h), the top plateaus of every dome
    that stands at least h above the saddle to higher ground (or has none inside its component), found by one reconstruction.
    With mask the flood stays inside it; with min_height only plateau cells with dsm > float32(min_height) count.
    -> (labels (gh, gw) int32, n, table, dome): the plateaus numbered by label(connectivity); table, from label_stats(): first
    int32 (n, 2) the (row, col) of every plateau's first cell in raster order, area int32 [cells], height float32, and with
    grid (a DSMGrid of that shape) east, north float64 of the first cell's centre; dome (gh, gw) float32 = dsm - h_maxima,
    exact (a multiple of 2^-8 m in 0 .. h), nodata where the DSM has no height.  The exact prominence of each peak is out of
    scope.  numpy if the DSM came as numpy, device tensors otherwise."""
    dsm = _hydro_dsm(dsm, grid)
    quanta = _h_quanta(h)
    connectivity = _connectivity_checked(connectivity)
    if min_height is not None:
        min_height = _finite(min_height, "min_height")
    mask = _domain_checked(mask, dsm.shape)
    z, as_numpy = _to_device(dsm)
    dev = z.device
    got = _seed_flood(z, z, _domain(mask, dev), float(nodata), -1, quanta, None, True, True)
    reached = got["steps"] >= 0
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    dome_q = torch.where(reached, torch.round(z.double() * 256.0) - torch.round(got["surface"].double() * 256.0), zero)
    top = reached & (dome_q == float(quanta))
    if min_height is not None:
        top &= z > float(np.float32(min_height))
    dome = torch.where(reached, (dome_q / 256.0).float(), torch.full_like(z, float(np.float32(nodata))))
    labels, n = label(top, connectivity)
    stats = label_stats(labels, n, values=z, nodata=nodata)
    first = _first_cells(labels, n)
    gw = z.shape[1]
    row, col = torch.div(first, gw, rounding_mode="floor"), first % gw
    table = {"first": torch.stack([row, col], dim=1).to(torch.int32), "area": stats["area"], "height": stats["max"]}
    if grid is not None:
        table["east"] = float(grid.e0) + col.double() * float(grid.xres)
        table["north"] = float(grid.n0) - row.double() * float(grid.yres)
    return _back(as_numpy, labels), n, {k: _back(as_numpy, t) for k, t in table.items()}, _back(as_numpy, dome)


def watershed(surface, markers, mask=None, peaks_up=True, nodata=-999.0, return_level=False):
    """The marker watershed of a surface (include/satmvs.h, "Seeded flood"): surface (gh, gw) float32, never converted; markers
    (gh, gw) int32, > 0 = a marker cell with that label (from peaks(), label(), or any map); mask as in reconstruct().  The
    surface is flooded from the marker cells at their own height, downwards from the peaks (peaks_up=True: objects on an nDSM)
    or upwards from the pits (False: catchment basins), every cell is reached over the lowest pass (the highest, peaks up), and
    ties go by the steps within a flat and then to the lowest neighbour number, so touching objects part along their saddles.
    The segments are basins() of the flood's back-links, each given the marker label at its root; the roots are the marker cells
    in row-major order.  -> (gh, gw) int32 in the markers' numbering, 0 where a cell is invalid, outside the mask or reached
    by no marker; with return_level also level (gh, gw) float32, the pass height at which the cell was reached (its own bits
    where that is the cell's height, nodata where the label is 0).  numpy if the surface came as numpy, device tensors
    otherwise."""
    surface = _hydro_dsm(surface)
    markers = _labels_checked(markers)
    if tuple(markers.shape) != tuple(surface.shape):
        raise ValueError("markers shape %s differs from the surface's %s" % (tuple(markers.shape), tuple(surface.shape)))
    mask = _domain_checked(mask, surface.shape)
    z, as_numpy = _to_device(surface)
    dev = z.device
    mk = _to_device(markers, dev=dev)[0]
    seeds = torch.where(mk > 0, z, torch.full_like(z, float("nan")))
    got = _seed_flood(z, seeds, _domain(mask, dev), float(nodata), -1 if peaks_up else 1, 0, None, return_level, False, True)
    basin, _ = basins(got["link"])
    roots = torch.nonzero(got["link"].reshape(-1) == 0)[:, 0]
    lut = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), mk.reshape(-1)[roots]])
    out = lut[basin.long()]
    return _back(as_numpy, out, got["surface"]) if return_level else _back(as_numpy, out)


def split_objects(above, grid, h=2.0, min_height=2.5, min_area_m2=50.0, connectivity=8, nodata=-999.0):
    """The objects of an nDSM, split where they merge: extract_objects(above, grid, min_height, min_area_m2) -> peaks(above, h,
    mask = objects > 0) -> watershed(above, peaks, mask = objects > 0), so that a terrace of houses, or a building and the trees
    that touch it, part along their saddles wherever both sides stand at least h above the saddle.  The segments are renumbered
    1 .. n in raster order of their first cells, label()'s numbering.  h = 2 m was chosen on a synthetic scene and is NOT tuned
    on real data; smoothing beforehand (focal_median()) is the caller's business: noise of more than h splits a roof.
    -> (labels (gh, gw) int32, n, table): table is label_stats(labels, n, values=above, grid=grid) plus `object` int32 (n), the
    label of extract_objects() under every segment.  outlines(), write_geojson() and label_quantiles() take the result as it
    is.  numpy if `above` came as numpy, device tensors otherwise."""
    above = _on_grid(_hydro_dsm(above), grid)
    _h_quanta(h)
    connectivity = _connectivity_checked(connectivity)
    min_height, min_area_m2 = _finite(min_height, "min_height"), _finite(min_area_m2, "min_area_m2")
    if min_area_m2 < 0.0:
        raise ValueError("min_area_m2 must be finite and >= 0, got %r" % min_area_m2)
    z, as_numpy = _to_device(above)
    objects, _ = extract_objects(z, grid, min_height, min_area_m2, connectivity, nodata)
    inside = objects > 0
    tops, n, _, _ = peaks(z, h, mask=inside, connectivity=connectivity, nodata=nodata)
    seg = watershed(z, tops, mask=inside, nodata=nodata)
    first = _first_cells(seg, n)
    order = torch.argsort(first)
    new_id = torch.zeros(n + 1, dtype=torch.int32, device=z.device)
    new_id[order + 1] = torch.arange(1, n + 1, dtype=torch.int32, device=z.device)
    labels = new_id[seg.long()]
    table = label_stats(labels, n, values=z, grid=grid, nodata=nodata)
    table["object"] = objects.reshape(-1)[first[order]]
    return _back(as_numpy, labels), n, {k: _back(as_numpy, t) for k, t in table.items()}


def open_by_reconstruction(dsm, radius, nodata=-999.0):
    """reconstruct(morph(dsm, radius, "open"), dsm): the opening that removes what a (2 radius + 1)^2 square does not fit into
    and does not round the corners of what it keeps.  -> (gh, gw) float32, as reconstruct()."""
    return reconstruct(morph(dsm, radius, "open", nodata), dsm, nodata=nodata)


# ---- meshes: the error-bounded triangulation of a DSM (adaptive RTIN), PLY and OBJ -----------------------------------------------
MAX_MESH_CELLS = 2 ** 29                                          # vertices and cells together in an int32 scan
MAX_MESH_TILE = 1024
MESH_INF = 2 ** 63 - 1                                            # the error of a vertex whose triangles hold a void or leave the grid
MESH_KEYS = ("vertices", "z", "triangles", "tri_level")


def _mesh_tile_checked(tile):
    tile = _int_checked(tile, "tile", 2, MAX_MESH_TILE)
    if tile & (tile - 1):
        raise ValueError("tile must be a power of two in 2 .. %d, got %r" % (MAX_MESH_TILE, tile))
    return tile


def _mesh_tol_units(tol):
    """tol [m] -> floor(256 tol), the tolerance in height quanta."""
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not math.isfinite(tol) or tol < 0:
        raise ValueError("tol is a finite number of metres >= 0, got %r" % (tol,))
    return int(math.floor(256.0 * float(tol)))


def _mesh_dsm(dsm, grid=None):
    dsm = _dsm_bits(dsm)
    if int(dsm.shape[0]) * int(dsm.shape[1]) >= MAX_MESH_CELLS:
        raise ValueError("meshes take fewer than 2^29 cells, got %d x %d" % (dsm.shape[0], dsm.shape[1]))
    if grid is not None:
        _on_grid(dsm, _grid_checked(grid, "grid"))
    return dsm


def _mesh_errors_checked(errors, dsm):
    """The int64 map of mesh_errors() for this DSM, never converted."""
    if isinstance(errors, torch.Tensor) != isinstance(dsm, torch.Tensor):
        raise ValueError("errors and dsm must both be numpy arrays or both be tensors")
    if not isinstance(errors, torch.Tensor):
        errors = np.asarray(errors)
    if errors.dtype not in (np.int64, torch.int64):
        raise ValueError("errors is int64, got %s" % (errors.dtype,))
    if tuple(errors.shape) != tuple(dsm.shape):
        raise ValueError("errors shape %s differs from the DSM's %s" % (tuple(errors.shape), tuple(dsm.shape)))
    return errors


def _mesh_inputs(dsm, grid, tol, tile, errors):
    """Everything checked before any device work -> z, as_numpy, the error map on the device, tol_units, the threshold."""
    dsm = _mesh_dsm(dsm, grid)
    tile = _mesh_tile_checked(tile)
    units = _mesh_tol_units(tol)
    if errors is not None:
        errors = _mesh_errors_checked(errors, dsm)
    z, as_numpy = _to_device(dsm)
    return z, as_numpy, errors, tile, units, min(units * tile, 2 ** 62)        # no finite error reaches 2^62


def _mesh_error_map(z, tile, nodata):
    gh, gw = z.shape
    e = torch.empty((gh, gw), dtype=torch.int64, device=z.device)
    _call(z.device, "smvs_dsm_mesh_errors", z, gw, gh, float(nodata), tile, e)
    return e


def mesh_errors(dsm, tile=256, nodata=-999.0):
    """The saturated error of every lattice vertex (include/satmvs.h smvs_dsm_mesh_errors, DESIGN.md section 9, "Meshes"): dsm
    (gh, gw) float32, fewer than 2^29 cells; tile a power of two in 2 .. 1024, the side S of the root squares.  -> int64
    (gh, gw) in units of 2^-8 m / S: the largest deviation of any lattice vertex from the plane of a triangle that the vertex
    splits, or of one further down that needs it; 2^63 - 1 where such a triangle holds a void or leaves the grid; 0 at the root
    squares' corners.  It depends on dsm, nodata and tile alone, bit for bit, and serves any number of tolerances: pass it to
    mesh() and mesh_heights() as `errors` for a chain of levels of detail.  numpy if the DSM came as numpy."""
    dsm = _mesh_dsm(dsm)
    tile = _mesh_tile_checked(tile)
    z, as_numpy = _to_device(dsm)
    return _back(as_numpy, _mesh_error_map(z, tile, nodata))


def _mesh_write(z, tile, nt, nv, ws, nbytes):
    """smvs_dsm_mesh_write into arrays of nt triangles and nv vertices -> the arrays and the status word, both on the device."""
    dev = z.device
    gh, gw = z.shape
    out = {"vertices": torch.empty((nv, 2), dtype=torch.int32, device=dev), "z": torch.empty(nv, dtype=torch.float32, device=dev),
           "triangles": torch.empty((nt, 3), dtype=torch.int32, device=dev), "tri_level": torch.empty(nt, dtype=torch.uint8, device=dev)}
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_mesh_write", z, gw, gh, tile, nt, nv, out["triangles"] if nt else None, out["tri_level"] if nt else None,
          out["vertices"] if nv else None, out["z"] if nv else None, status, ws, nbytes)
    return out, status


def _mesh_status_checked(status, nt, nv):
    """One host read: the write's status is n_triangles, or -1 where the counts given were not the workspace's."""
    if int(status.item()) != nt:
        raise _lib.SatMVSNativeError("smvs_dsm_mesh_write gave up: %d triangles and %d vertices are not the counts of its workspace" % (nt, nv))


def mesh(dsm, grid=None, tol=0.5, tile=256, nodata=-999.0, errors=None):
    """A triangle mesh of a DSM with a guaranteed error (include/satmvs.h smvs_dsm_mesh_count / _write, DESIGN.md section 9,
    "Meshes"): the right-triangulated irregular network over the lattice of cell centres, refined exactly where a triangle's
    plane would leave some lattice height by more than tol.  dsm (gh, gw) float32; tol [m] >= 0, used as floor(256 tol) height
    quanta of 2^-8 m (tol = 0: lossless in the quantised heights); tile as in mesh_errors(); errors: that function's result for
    this dsm, nodata and tile, else it is computed here.  Every lattice height within a triangle lies within tol of its plane;
    the mesh has no T-junctions and covers exactly the finest half-cells whose three corners hold a height (voids and the
    grid's outside are holes).
    -> dict: vertices int32 (V, 2) col, row, in row-major order; z float32 (V), the DSM's own bits; triangles int32 (T, 3)
      indices a, b, c, hypotenuse a -> b and right angle at c, counter-clockwise seen from above (east right, north up), sorted
      by (row, col) of a + b and the apex's side; tri_level uint8 (T), 0 the root triangles .. 2 log2(tile) the half-cells;
      n_vertices, n_triangles, tile, tol_units as Python ints; with grid (a DSMGrid of the DSM's shape) xyz float64 (V, 3): east,
      north of the cell centres (e0 + col xres, n0 - row yres) and z.
    numpy if the DSM came as numpy, device tensors otherwise.  The host reads the device once, for the two counts, like
    outlines(); the write is given those very counts, so its status (-1 for counts that are not the workspace's) can only tell
    of a workspace damaged in between: it is read and raised for numpy, whose arrays go to the host anyway, and not for tensors."""
    z, as_numpy, errors, tile, units, thr = _mesh_inputs(dsm, grid, tol, tile, errors)
    dev = z.device
    gh, gw = z.shape
    e = _mesh_error_map(z, tile, nodata) if errors is None else _to_device(errors, dev=dev)[0]
    nbytes = _lib.load().smvs_dsm_mesh_workspace_bytes(gw, gh, tile)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _call(dev, "smvs_dsm_mesh_count", e, z, gw, gh, float(nodata), tile, thr, counts, ws, nbytes)
    nt, nv = counts.tolist()
    out, status = _mesh_write(z, tile, nt, nv, ws, nbytes)
    if as_numpy:                                             # everything goes to the host anyway; tensors: see the docstring
        _mesh_status_checked(status, nt, nv)
    if grid is not None:
        v = out["vertices"].double()
        out["xyz"] = torch.stack([float(grid.e0) + v[:, 0] * float(grid.xres), float(grid.n0) - v[:, 1] * float(grid.yres), out["z"].double()], dim=1)
    out = {k: _back(as_numpy, t) for k, t in out.items()}
    out.update(n_vertices=nv, n_triangles=nt, tile=tile, tol_units=units)
    return out


def mesh_heights(dsm, tol, tile=256, nodata=-999.0, errors=None, return_dev=False):
    """The height of mesh(dsm, tol=tol, tile=tile) at every lattice vertex (include/satmvs.h smvs_dsm_mesh_heights): float32
    (gh, gw), fl32(S plane / (256 S)) with one IEEE division, nodata where the vertex is a void or in no triangle; a mesh vertex
    gets its own quantised height.  return_dev: also int64 S q - S plane in the errors' units (|dev| <= floor(256 tol) tile at
    every covered vertex, 0 at the mesh's vertices, 2^63 - 1 where uncovered).  To compare a mesh with its DSM without
    rasterising triangles."""
    z, as_numpy, errors, tile, units, thr = _mesh_inputs(dsm, None, tol, tile, errors)
    dev = z.device
    gh, gw = z.shape
    e = _mesh_error_map(z, tile, nodata) if errors is None else _to_device(errors, dev=dev)[0]
    nbytes = _lib.load().smvs_dsm_mesh_workspace_bytes(gw, gh, tile)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    h = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    d = torch.empty((gh, gw), dtype=torch.int64, device=dev) if return_dev else None
    _call(dev, "smvs_dsm_mesh_heights", e, z, gw, gh, float(nodata), tile, thr, h, d, ws, nbytes)
    return _back(as_numpy, h, d) if return_dev else _back(as_numpy, h)


def _mesh_host(mesh, grid):
    """vertices, z, triangles of a mesh() dict as host arrays and its (V, 3) float64 east, north, z on `grid`."""
    for key in MESH_KEYS:
        if key not in mesh:
            raise ValueError("mesh is the dict of mesh(): entry %r is missing" % key)
    host = {k: (mesh[k].cpu().numpy() if hasattr(mesh[k], "cpu") else np.asarray(mesh[k])) for k in MESH_KEYS}
    v, z, t = host["vertices"], host["z"], host["triangles"]
    if v.ndim != 2 or v.shape[1] != 2 or z.shape != (len(v),) or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("mesh is the dict of mesh()")
    _grid_checked(grid, "grid")
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("mesh holds a triangle index outside its vertices")
    if len(v) and (v.min() < 0 or v[:, 0].max() >= int(grid.width) or v[:, 1].max() >= int(grid.height)):
        raise ValueError("mesh holds a vertex outside the grid")
    xyz = np.stack([float(grid.e0) + v[:, 0].astype(np.float64) * float(grid.xres),
                    float(grid.n0) - v[:, 1].astype(np.float64) * float(grid.yres), z.astype(np.float64)], axis=1)
    return v, t.astype("<i4"), xyz


def write_ply(path, mesh, grid, colors=None):
    """A mesh() dict as a binary little-endian PLY: vertices x (east), y (north), z as float64, faces as lists of three int32.
    float64 rather than float32 offsets from a `comment origin`: map coordinates need 7 to 8 digits before the decimal point,
    double properties are plain PLY that the common readers take, and a reader that ignores comments still gets the right
    coordinates.  colors: a uint8 (gh, gw, 3) image on the DSM's grid (an orthophoto of orthorectify(), say), read at the
    vertices into red, green, blue.  Standard library and numpy only.  -> the number of faces."""
    v, t, xyz = _mesh_host(mesh, grid)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    if colors is not None:
        colors = np.asarray(colors.cpu() if hasattr(colors, "cpu") else colors)
        if colors.dtype != np.uint8 or colors.shape != (int(grid.height), int(grid.width), 3):
            raise ValueError("colors is a uint8 (%d, %d, 3) image on the grid, got %s %s" % (grid.height, grid.width, colors.dtype, colors.shape))
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(len(v), dtype=fields)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if colors is not None:
        at = colors[v[:, 1], v[:, 0]]
        rec["red"], rec["green"], rec["blue"] = at[:, 0], at[:, 1], at[:, 2]
    faces = np.empty(len(t), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"], faces["v"] = 3, t
    names = {"<f8": "double", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", "comment DSM mesh: east north height, tile %d, tol_units %d" % (
        int(mesh.get("tile", 0)), int(mesh.get("tol_units", 0))), "element vertex %d" % len(v)]
    header += ["property %s %s" % (names[kind], name) for name, kind in fields]
    header += ["element face %d" % len(t), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())
    return len(t)


def write_obj(path, mesh, grid, texcoords=False):
    """A mesh() dict as a Wavefront OBJ in plain text: `v east north z` with every digit of the float64, then with texcoords
    `vt col / (gw - 1)  1 - row / (gh - 1)` (the orthophoto on the same grid as the texture image, its first row on top), then
    `f a b c` or `f a/a b/b c/c`, indices from 1.  Standard library and numpy only.  -> the number of faces."""
    v, t, xyz = _mesh_host(mesh, grid)
    gw1, gh1 = max(int(grid.width) - 1, 1), max(int(grid.height) - 1, 1)
    with open(path, "w") as f:
        f.write("# DSM mesh: %d vertices, %d faces\n" % (len(v), len(t)))
        for x, y, z in xyz.tolist():
            f.write("v %r %r %r\n" % (x, y, z))
        if texcoords:
            for col, row in v.tolist():
                f.write("vt %r %r\n" % (col / gw1, 1.0 - row / gh1))
        form = "f %d/%d %d/%d %d/%d\n" if texcoords else "f %d %d %d\n"
        for a, b, c in (t + 1).tolist():
            f.write(form % ((a, a, b, b, c, c) if texcoords else (a, b, c)))
    return len(t)


# ---- registration: one DSM onto another's grid, the shift between two DSMs, scores and changes ---------------------------------
REGRID_MODES = {"nearest": 0, "bilinear": 1}
MAX_SHIFT_RADIUS = 32
MAX_TRIM = 256.0


def _grid_checked(grid, name):
    vals = (grid.e0, grid.n0, grid.xres, grid.yres)
    if not all(math.isfinite(float(v)) for v in vals) or not (float(grid.xres) > 0.0 and float(grid.yres) > 0.0):
        raise ValueError("%s needs finite origins and positive finite resolutions, got %r" % (name, grid))
    gw, gh = int(grid.width), int(grid.height)
    if gw < 1 or gh < 1 or gw * gh >= 2 ** 31:
        raise ValueError("%s has positive sizes and fewer than 2^31 cells, got %d x %d" % (name, gw, gh))
    return grid


def _finite(v, name):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError("%s must be finite, got %r" % (name, v))
    return v


def _trim_checked(trim):
    trim = float(trim)
    if not (0.0 < trim <= MAX_TRIM):
        raise ValueError("trim must be in (0, %g] m, got %r" % (MAX_TRIM, trim))
    return trim


def regrid(dsm, grid, to_grid, mode="bilinear", dz=0.0, nodata=-999.0):
    """A DSM on `grid` resampled onto `to_grid` (include/satmvs.h smvs_dsm_regrid, DESIGN.md section 9, "Registration"): every
    cell of to_grid takes the source cell its centre falls in ("nearest") or the bilinear mean of the four around it
    ("bilinear", float64), plus dz [m]; a tap that is off the grid or invalid makes the cell nodata, and a tap with the
    weight 0 is not read, so onto a grid whose centres coincide with the source's the result is a crop, bit for bit with
    dz = 0.  dsm (grid.height, grid.width) of any real dtype (taken as float32), numpy or a device tensor.
    -> (to_grid.height, to_grid.width) float32; numpy if the DSM came as numpy, a device tensor otherwise."""
    if mode not in REGRID_MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(REGRID_MODES), mode))
    _grid_checked(grid, "grid")
    _grid_checked(to_grid, "to_grid")
    dz = _finite(dz, "dz")
    dsm = _dsm_converted(dsm, grid)
    z, as_numpy = _to_device(dsm, torch.float32)
    out = torch.empty((int(to_grid.height), int(to_grid.width)), dtype=torch.float32, device=z.device)
    _call(z.device, "smvs_dsm_regrid", z, int(grid.width), int(grid.height), grid.grid4(), float(nodata), to_grid.grid4(),
          int(to_grid.width), int(to_grid.height), REGRID_MODES[mode], dz, out)
    return _back(as_numpy, out)


def shift_stats(a, b, offset=(0, 0), radius=8, dz0=0.0, trim=256.0, nodata=-999.0):
    """The statistics of a - b under every integer shift (include/satmvs.h smvs_dsm_shift_stats): for (sx, sy) in [-radius,
    radius]^2 cell (r, c) of b meets cell (r + oy + sy, c + ox + sx) of a, offset = (ox, oy); d = a - b - dz0 in float64; the
    pair counts iff both cells are valid and |d| <= trim [m]; q = d in units of 2^-8 m, rounded half to even.
    a, b: (gh, gw) float32 grids of equal cell size, numpy or device tensors, never converted; 0 <= radius <= 32; 0 < trim <= 256.
    -> (2 radius + 1, 2 radius + 1, 3) int64, [sy + radius, sx + radius] = (n, sum q, sum q^2), exact integer sums with
    equal bits from run to run; numpy if `a` came as numpy, a device tensor otherwise."""
    a, b = _dsm_bits(a), _dsm_bits(b)
    ox, oy = _int_pair(offset, "offset")
    if abs(ox) >= 2 ** 30 or abs(oy) >= 2 ** 30:
        raise ValueError("offset must be below 2^30 in size, got %r" % ((ox, oy),))
    radius = _int_checked(radius, "radius", 0, MAX_SHIFT_RADIUS)
    dz0 = _finite(dz0, "dz0")
    trim = _trim_checked(trim)
    za, as_numpy = _to_device(a)
    zb, _ = _to_device(b, dev=za.device)
    (gha, gwa), (ghb, gwb) = za.shape, zb.shape
    nbytes = _lib.load().smvs_dsm_shift_workspace_bytes(gwa, gha, gwb, ghb, radius)
    if nbytes == 0:
        raise ValueError("unsupported shift search: %d x %d against %d x %d cells, radius %d" % (gwa, gha, gwb, ghb, radius))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=za.device)
    side = 2 * radius + 1
    stats = torch.empty((side, side, 3), dtype=torch.int64, device=za.device)
    _call(za.device, "smvs_dsm_shift_stats", za, gwa, gha, zb, gwb, ghb, float(nodata), ox, oy, radius, dz0, trim, stats, ws, nbytes)
    return _back(as_numpy, stats)


def best_shift(stats, min_overlap=0.5):
    """The selection rule of coregister on one (2R + 1, 2R + 1, 3) array of shift_stats, on the host in exact Python integers:
    a shift is eligible iff n >= max(2, ceil(min_overlap max n)); the best is the eligible one with the lowest variance
    (n sum q^2 - (sum q)^2) / n^2, compared by cross-multiplication; ties go to the smaller sx^2 + sy^2, then the lower sy,
    then the lower sx.  The sub-cell step per axis is the vertex of the parabola through the variances at the best shift and
    its two neighbours, d = (c- - c+) / (2 (c- - 2 c0 + c+)) in float64 clamped to +-1/2, 0 where a neighbour is missing or not
    eligible or the denominator is <= 0.
    -> None if no shift is eligible, else dict: shift (sx, sy), subcell (dx, dy), n, sum_q, variance_q (float64, in q^2)."""
    st = np.asarray(stats.detach().cpu() if isinstance(stats, torch.Tensor) else stats)
    if st.ndim != 3 or st.shape[0] != st.shape[1] or st.shape[0] % 2 != 1 or st.shape[2] != 3:
        raise ValueError("stats is (2R + 1, 2R + 1, 3), got %s" % (tuple(st.shape),))
    min_overlap = float(min_overlap)
    if not 0.0 <= min_overlap <= 1.0:
        raise ValueError("min_overlap must be in 0 .. 1, got %r" % min_overlap)
    R = st.shape[0] // 2
    rows = st.tolist()                                        # Python integers from here on
    need = max(2, int(math.ceil(min_overlap * max(max(v[0] for v in row) for row in rows))))

    def cost(sx, sy):
        """(numerator, denominator) of the variance of an eligible shift on the grid, else None."""
        if abs(sx) > R or abs(sy) > R:
            return None
        n, s1, s2 = rows[sy + R][sx + R]
        return (n * s2 - s1 * s1, n * n) if n >= need else None

    best = None
    for sy in range(-R, R + 1):
        for sx in range(-R, R + 1):
            c = cost(sx, sy)
            if c is None:
                continue
            key = (sx * sx + sy * sy, sy, sx)
            if best is None:
                lower = True
            else:
                lhs, rhs = c[0] * best[0][1], best[0][0] * c[1]
                lower = lhs < rhs or (lhs == rhs and key < best[1])
            if lower:
                best = (c, key)
    if best is None:
        return None
    (num, den), (_, sy, sx) = best

    def vertex(lo, hi):
        if lo is None or hi is None:
            return 0.0
        c0, cl, ch = num / den, lo[0] / lo[1], hi[0] / hi[1]
        bend = cl - 2.0 * c0 + ch
        return min(0.5, max(-0.5, 0.5 * (cl - ch) / bend)) if bend > 0.0 else 0.0

    n, s1, _ = rows[sy + R][sx + R]
    return {"shift": (sx, sy), "subcell": (vertex(cost(sx - 1, sy), cost(sx + 1, sy)), vertex(cost(sx, sy - 1), cost(sx, sy + 1))),
            "n": n, "sum_q": s1, "variance_q": num / den}


def coregister(a, grid_a, b, grid_b, radius=8, trim=10.0, min_overlap=0.5, rounds=2, nodata=-999.0):
    """The offset between two DSMs of equal cell size: the planimetric shift, in whole cells within +-radius of where the
    georeferences put them, that minimises the variance of a - b, refined to a fraction of a cell by a parabola per axis,
    and the vertical offset from the mean (best_shift for the rule).  Round 1 runs shift_stats with dz0 = 0 and trim = 256 m;
    every later round with dz0 = the last dz and the caller's trim [m], which keeps changes and blunders out of the sums.
    The defaults (radius 8, trim 10 m, two rounds) are a choice for 5 m grids on a synthetic scene, not tuned
    on real data.  a is the moving DSM, b the fixed one; both (gh, gw) float32, never converted.
    -> dict: shift_cells (sx, sy): b's cell (r, c) meets a's cell (r + oy + sy, c + ox + sx); subcell (dx, dy) in cells;
    de, dn [m]: what to add to a's georeference; grid: grid_a moved by (de, dn) -- nothing is resampled, registration changes
    the world file; dz [m] = dz0 + sum q / (256 n): the mean of a - b over the counted pairs, so a - dz meets b
    (regrid(a, grid, grid_b, dz=-dz)); n; std [m] of a - b at the best shift; offset (ox, oy); stats: the last round's
    shift_stats.  Raises ValueError("no overlap") when no shift has two pairs."""
    a, b = _on_grid(_dsm_bits(a), grid_a), _on_grid(_dsm_bits(b), grid_b)
    _grid_checked(grid_a, "grid_a")
    _grid_checked(grid_b, "grid_b")
    if float(grid_a.xres) != float(grid_b.xres) or float(grid_a.yres) != float(grid_b.yres):
        raise ValueError("coregister needs grids of equal xres and equal yres (%r, %r against %r, %r): regrid() one DSM onto "
                         "the other's resolution first" % (grid_a.xres, grid_a.yres, grid_b.xres, grid_b.yres))
    radius = _int_checked(radius, "radius", 0, MAX_SHIFT_RADIUS)
    rounds = _int_checked(rounds, "rounds", 1, 16)
    trim = _trim_checked(trim)
    min_overlap = float(min_overlap)
    if not 0.0 <= min_overlap <= 1.0:
        raise ValueError("min_overlap must be in 0 .. 1, got %r" % min_overlap)
    xres, yres = float(grid_a.xres), float(grid_a.yres)
    u0, v0 = (float(grid_b.e0) - float(grid_a.e0)) / xres, (float(grid_a.n0) - float(grid_b.n0)) / yres
    ox, oy = math.floor(u0 + 0.5), math.floor(v0 + 0.5)      # b's cell (0, 0) in a's index space, to the nearest cell
    if abs(ox) >= 2 ** 30 or abs(oy) >= 2 ** 30:
        raise ValueError("no overlap")
    fx, fy = u0 - ox, v0 - oy                                # what the rounding left, carried into de and dn
    dz, pick, stats = 0.0, None, None
    for k in range(rounds):
        stats = shift_stats(a, b, (ox, oy), radius, dz, 256.0 if k == 0 else trim, nodata)
        pick = best_shift(stats, min_overlap)
        if pick is None:
            raise ValueError("no overlap")
        dz = dz + pick["sum_q"] / (256.0 * pick["n"])
    (sx, sy), (dx, dy) = pick["shift"], pick["subcell"]
    de, dn = (fx - sx - dx) * xres, (sy + dy - fy) * yres
    moved = DSMGrid(float(grid_a.e0) + de, float(grid_a.n0) + dn, grid_a.xres, grid_a.yres, grid_a.width, grid_a.height)
    return {"shift_cells": (sx, sy), "subcell": (dx, dy), "de": de, "dn": dn, "dz": dz, "n": pick["n"],
            "std": math.sqrt(max(pick["variance_q"], 0.0)) / 256.0, "grid": moved, "offset": (ox, oy), "stats": stats}


def _same_resolution(g, h):
    return float(g.xres) == float(h.xres) and float(g.yres) == float(h.yres)


def _registered(a, grid_a, b, grid_b, register, nodata, **coregister_kw):
    """(a on grid_b as the georeferences say, a on grid_b after registration, the coregister dict or None)."""
    plain = regrid(a, grid_a, grid_b, nodata=nodata)
    if not register:
        return plain, plain, None
    if _same_resolution(grid_a, grid_b):
        a32 = a.to(torch.float32) if isinstance(a, torch.Tensor) else np.asarray(a, np.float32)
        shift = coregister(a32, grid_a, b, grid_b, nodata=nodata, **coregister_kw)
    else:                                                    # the nearest grid of b's resolution is b's own
        shift = coregister(plain, grid_b, b, grid_b, nodata=nodata, **coregister_kw)
    moved = DSMGrid(float(grid_a.e0) + shift["de"], float(grid_a.n0) + shift["dn"], grid_a.xres, grid_a.yres, grid_a.width, grid_a.height)
    shift = dict(shift, grid=moved)
    return plain, regrid(a, moved, grid_b, dz=-shift["dz"], nodata=nodata), shift


def compare_dsms(est, grid_est, gt, grid_gt, register=True, nodata=-999.0, thresholds=(2.5, 7.5), **coregister_kw):
    """Score a DSM against a reference DSM on another grid: est is regridded (bilinear) onto grid_gt and scored with dsm_metrics
    ("before"); with `register` the offset between the two is found with coregister (on est itself where the resolutions are
    equal, else on est regridded onto grid_gt), est is regridded again from the corrected grid with -dz, and scored ("after").
    gt (grid_gt's shape) float32.  -> {"shift": the coregister dict (None without register), "before": ..., "after": ...}."""
    _on_grid(gt, grid_gt)
    plain, moved, shift = _registered(est, grid_est, gt, grid_gt, register, nodata, **coregister_kw)
    g = torch.as_tensor(gt).to(plain.device) if isinstance(plain, torch.Tensor) else torch.as_tensor(np.asarray(gt))
    before = dsm_metrics(torch.as_tensor(plain), g, float(np.float32(nodata)), thresholds)
    after = dsm_metrics(torch.as_tensor(moved), g, float(np.float32(nodata)), thresholds) if register else before
    return {"shift": shift, "before": before, "after": after}


def compare_dsms_robust(est, grid_est, gt, grid_gt, register=True, nodata=-999.0, levels=(0.6827, 0.9, 0.95), **coregister_kw):
    """compare_dsms with dsm_metrics_robust in the place of dsm_metrics: the median error, NMAD and LE68 / LE90 / LE95 of est
    against gt before and after the registration.  -> {"shift", "before", "after"} as compare_dsms gives them."""
    _on_grid(gt, grid_gt)
    plain, moved, shift = _registered(est, grid_est, gt, grid_gt, register, nodata, **coregister_kw)
    before = dsm_metrics_robust(plain, gt, nodata, levels)
    after = dsm_metrics_robust(moved, gt, nodata, levels) if register else before
    return {"shift": shift, "before": before, "after": after}


def changes(a, grid_a, b, grid_b, min_dh=2.5, min_area_m2=50.0, register=True, connectivity=8, nodata=-999.0, **coregister_kw):
    """What changed between two epochs: a is registered to b (coregister, unless register=False) and regridded onto grid_b;
    diff = a - b in float32 where both are valid, nodata elsewhere; the rises (diff > min_dh) and the falls (-diff > min_dh)
    each go through extract_objects with min_area_m2, and the falls' labels are numbered after the rises'.
    -> (diff (grid_b's shape) float32, labels int32, stats: extract_objects' dict over rises then falls, heights as |diff|,
    plus sign int8 (+1 rise, -1 fall)); numpy if `a` came as numpy, device tensors otherwise."""
    _on_grid(b, grid_b)
    _, moved, _ = _registered(a, grid_a, b, grid_b, register, nodata, **coregister_kw)
    as_numpy = not isinstance(moved, torch.Tensor)
    za, _ = _to_device(moved)
    zb, _ = _to_device(b if isinstance(b, torch.Tensor) else np.asarray(b, np.float32), torch.float32, za.device)
    nd = float(np.float32(nodata))
    both = torch.isfinite(za) & (za != nd) & torch.isfinite(zb) & (zb != nd)
    d = za - zb
    diff = torch.where(both, d, torch.full_like(d, nd))
    up_labels, up = extract_objects(diff, grid_b, min_dh, min_area_m2, connectivity, nodata)
    down_labels, down = extract_objects(torch.where(both, -d, torch.full_like(d, nd)), grid_b, min_dh, min_area_m2, connectivity, nodata)
    n_up = int(up["area"].numel())
    labels = up_labels + torch.where(down_labels > 0, down_labels + n_up, torch.zeros_like(down_labels))
    stats = {k: torch.cat([up[k], down[k]]) for k in up}
    stats["sign"] = torch.cat([torch.ones(n_up, dtype=torch.int8, device=za.device),
                               -torch.ones(int(down["area"].numel()), dtype=torch.int8, device=za.device)])
    return _back(as_numpy, diff), _back(as_numpy, labels), {k: _back(as_numpy, v) for k, v in stats.items()}


# ---- mosaic: the distance to the nearest void or edge, and tiles on one lattice blended into one DSM ----------------------------
MAX_DIST = 1024
MAX_MOSAIC_LAYERS = 64
MOSAIC_MODES = {"first": 0, "last": 1, "min": 2, "max": 3, "mean": 4, "feather": 5}
ALIGN_TOLERANCE = 1e-6                                            # cells; see mosaic()


class _Layer(ctypes.Structure):                                   # smvs_dsm_layer of include/satmvs.h
    _fields_ = [("z", ctypes.c_void_p), ("d2", ctypes.c_void_p), ("gw", ctypes.c_int), ("gh", ctypes.c_int),
                ("ox", ctypes.c_int), ("oy", ctypes.c_int)]


def _mask_u8(mask):
    """A checked mask as a contiguous uint8 device tensor of 0 / 1 -> (tensor, whether the caller gave numpy)."""
    mask = _mask_checked(mask)
    if not isinstance(mask, torch.Tensor):
        mask = np.not_equal(mask, 0).view(np.uint8)
    m, as_numpy = _to_device(mask)
    return (m != 0).to(torch.uint8).contiguous(), as_numpy


def _dist(m, max_dist, border):
    """smvs_dsm_dist of a uint8 device mask -> (gh, gw) int32 device tensor."""
    gh, gw = m.shape
    nbytes = _lib.load().smvs_dsm_dist_workspace_bytes(gw, gh, max_dist)
    if nbytes == 0:
        raise ValueError("unsupported distance transform: %d x %d cells, max_dist %d" % (gw, gh, max_dist))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    d2 = torch.empty((gh, gw), dtype=torch.int32, device=m.device)
    _call(m.device, "smvs_dsm_dist", m, gw, gh, 1 if border else 0, max_dist, d2, ws, nbytes)
    return d2


def _max_dist_checked(max_dist, shape):
    if max_dist is None:
        return min(MAX_DIST, int(math.ceil(math.hypot(int(shape[0]), int(shape[1])))))
    return _int_checked(max_dist, "max_dist", 1, MAX_DIST)


def distance(mask, max_dist=None, border=False, squared=False):
    """The exact Euclidean distance of every cell to the nearest background cell (include/satmvs.h smvs_dsm_dist, DESIGN.md
    section 9, "Mosaic"): mask (gh, gw), bool or an integer dtype, numpy or a device tensor, non-zero = foreground; the
    background is the zero cells and, with `border`, everything off the grid.  Distances are capped at max_dist cells
    (1 .. 1024; None = min(1024, ceil(hypot(gh, gw))), which no distance within the grid exceeds): a value equal to max_dist
    means "at least max_dist", also where there is no background cell at all.
    -> (gh, gw) int32 squared distances with `squared` (scipy.ndimage.distance_transform_edt(mask)^2, capped, bit for bit), else
    their float32 square roots in cells; numpy if the mask came as numpy, a device tensor otherwise."""
    mask = _mask_checked(mask)
    max_dist = _max_dist_checked(max_dist, mask.shape)
    m, as_numpy = _mask_u8(mask)
    d2 = _dist(m, max_dist, border)
    return _back(as_numpy, d2 if squared else d2.to(torch.float64).sqrt().to(torch.float32))


def _radius_cap(radius):
    """(floor(radius^2), the transform's cap) of a buffer radius, checked."""
    radius = float(radius)
    if not (0.0 < radius < float(MAX_DIST)):
        raise ValueError("radius must be above 0 and below %d cells (at %d the transform's cap could not tell 'exactly' from "
                         "'further'), got %r" % (MAX_DIST, MAX_DIST, radius))
    return int(math.floor(radius * radius)), int(math.floor(radius)) + 1


def buffer_mask(mask, radius, border=False):
    """The Euclidean buffer of a mask: True where a set cell lies within `radius` cells, inclusive (the set cells themselves
    are True), as the integer comparison d^2 <= floor(radius^2) on distance(~mask, floor(radius) + 1, border, squared=True).
    With `border` everything off the grid counts as set.  0 < radius < 1024.
    -> (gh, gw) bool; numpy if the mask came as numpy, a device tensor otherwise."""
    mask = _mask_checked(mask)
    limit, cap = _radius_cap(radius)
    m, as_numpy = _mask_u8(mask)
    return _back(as_numpy, _dist(1 - m, cap, border) <= limit)


def _layer_offset(grid, to_grid):
    """Where cell (0, 0) of `grid` lies on `to_grid`, from the world-file numbers in float64 -> (ox, oy, aligned)."""
    u = (float(grid.e0) - float(to_grid.e0)) / float(to_grid.xres)
    v = (float(to_grid.n0) - float(grid.n0)) / float(to_grid.yres)
    ox, oy = math.floor(u + 0.5), math.floor(v + 0.5)
    aligned = _same_resolution(grid, to_grid) and abs(u - ox) <= ALIGN_TOLERANCE and abs(v - oy) <= ALIGN_TOLERANCE
    return int(ox), int(oy), aligned


def _span_on(grid, to_grid):
    """The first and last column and row of to_grid's lattice (unclipped) that the cell centres of `grid` reach."""
    ox, oy, aligned = _layer_offset(grid, to_grid)
    if aligned:
        return ox, ox + int(grid.width) - 1, oy, oy + int(grid.height) - 1
    u0 = (float(grid.e0) - float(to_grid.e0)) / float(to_grid.xres)
    v0 = (float(to_grid.n0) - float(grid.n0)) / float(to_grid.yres)
    u1 = u0 + (int(grid.width) - 1) * float(grid.xres) / float(to_grid.xres)
    v1 = v0 + (int(grid.height) - 1) * float(grid.yres) / float(to_grid.yres)
    return math.floor(u0), math.ceil(u1), math.floor(v0), math.ceil(v1)


def _grids_checked(grids):
    grids = list(grids)
    if not grids:
        raise ValueError("a mosaic needs at least one layer")
    if len(grids) > MAX_MOSAIC_LAYERS:
        raise ValueError("a mosaic takes at most %d layers, got %d: mosaic them in groups" % (MAX_MOSAIC_LAYERS, len(grids)))
    return [_grid_checked(g, "grids[%d]" % k) for k, g in enumerate(grids)]


def mosaic_grid(grids):
    """The smallest DSMGrid on the lattice of grids[0] (its origin and cell sizes) that covers the cell centres of every grid."""
    grids = _grids_checked(grids)
    first = grids[0]
    spans = [_span_on(g, first) for g in grids]
    c0, c1 = min(s[0] for s in spans), max(s[1] for s in spans)
    r0, r1 = min(s[2] for s in spans), max(s[3] for s in spans)
    out = DSMGrid(float(first.e0) + c0 * float(first.xres), float(first.n0) - r0 * float(first.yres), first.xres, first.yres,
                  int(c1 - c0 + 1), int(r1 - r0 + 1))
    return _grid_checked(out, "the mosaic's grid")


def _align_checked(align):
    if align is not None and align not in REGRID_MODES:
        raise ValueError("align must be None or one of %s, got %r" % (sorted(REGRID_MODES), align))
    return align


def _plan_layers(dsms, grids, to_grid, align):
    """Where the layers of a mosaic or a stack lie on the destination's lattice, as mosaic() states it; to_grid=None means
    mosaic_grid(grids).  Host work only: every check is made before a device is asked for.
    -> (to_grid, dsms, grids, plan), plan[k] = (ox, oy, None) of an aligned layer, (c0, r0, the sub-grid of to_grid's lattice to
    regrid onto) of an unaligned one."""
    dsms = list(dsms)
    grids = _grids_checked(grids)
    if len(dsms) != len(grids):
        raise ValueError("one grid per DSM: %d DSMs, %d grids" % (len(dsms), len(grids)))
    to_grid = mosaic_grid(grids) if to_grid is None else _grid_checked(to_grid, "to_grid")
    gw, gh = int(to_grid.width), int(to_grid.height)
    dsms = [_dsm_converted(z, g) for z, g in zip(dsms, grids)]
    plan = []                                                # per layer: (ox, oy, None) or (c0, r0, the sub-grid to regrid onto)
    for k, g in enumerate(grids):
        ox, oy, aligned = _layer_offset(g, to_grid)
        if aligned:
            if abs(ox) >= 2 ** 30 or abs(oy) >= 2 ** 30:
                raise ValueError("grids[%d] lies %d, %d cells from to_grid: offsets must be below 2^30" % (k, ox, oy))
            plan.append((ox, oy, None))
            continue
        if align is None:
            raise ValueError("grids[%d] is not aligned with to_grid (equal cell sizes and an offset within %g cell of whole cells): "
                             "pass align='nearest' or 'bilinear', or regrid() it yourself" % (k, ALIGN_TOLERANCE))
        c0, c1, r0, r1 = _span_on(g, to_grid)
        c0, c1, r0, r1 = max(c0, 0), min(c1, gw - 1), max(r0, 0), min(r1, gh - 1)
        if c1 < c0 or r1 < r0:                               # misses the destination: one void cell stands for it
            c0 = c1 = r0 = r1 = 0
        sub = DSMGrid(float(to_grid.e0) + c0 * float(to_grid.xres), float(to_grid.n0) - r0 * float(to_grid.yres),
                      to_grid.xres, to_grid.yres, c1 - c0 + 1, r1 - r0 + 1)
        plan.append((c0, r0, sub))
    return to_grid, dsms, grids, plan


def _place_layers(dsms, grids, plan, align, nodata):
    """The planned layers on the device, an unaligned one regrid()ded by `align` onto its sub-grid.
    -> (dev, as_numpy, [(z float32 device tensor, ox, oy)]); the caller keeps the tensors alive until its call is enqueued."""
    as_numpy = not isinstance(dsms[0], torch.Tensor)
    dev = _dev() if as_numpy or not dsms[0].is_cuda else dsms[0].device
    layers = []
    for z, g, (ox, oy, sub) in zip(dsms, grids, plan):
        z, _ = _to_device(z, torch.float32, dev)
        if sub is not None:
            z = regrid(z, g, sub, mode=align, nodata=nodata)
        layers.append((z, ox, oy))
    return dev, as_numpy, layers


def _layer_table(layers, d2=None):
    """The smvs_dsm_layer records of _plan_layers()'s layers, d2[k] (or none) beside each."""
    table = (_Layer * len(layers))()
    for k, (z, ox, oy) in enumerate(layers):
        table[k] = _Layer(z.data_ptr(), d2[k].data_ptr() if d2 is not None else None, int(z.shape[1]), int(z.shape[0]), ox, oy)
    return table


def mosaic(dsms, grids, to_grid=None, mode="feather", feather=16, align=None, nodata=-999.0,
           return_count=False, return_source=False, return_spread=False):
    """Several DSMs put together on one grid (include/satmvs.h smvs_dsm_mosaic, DESIGN.md section 9, "Mosaic").  dsms[k] is
    (grids[k].height, grids[k].width) of any real dtype (taken as float32), numpy or a device tensor; at most 64 layers;
    to_grid=None means mosaic_grid(grids).  Where several layers are valid a destination cell takes, by `mode`, the "first" or
    "last" of them in the list's order, the "min" or "max" (ties to the earlier layer), their "mean" (float64, in the list's
    order), or the "feather" blend: the mean with the weights min(max(d, 1), feather), d the distance [cells] of the layer's
    cell to the layer's nearest void or edge (smvs_dsm_dist of its validity mask with the border as background), so a tile
    fades out over `feather` cells towards its seams instead of leaving a step there.  Cells no layer covers get nodata; one
    layer alone comes back bit for bit in every mode.
    A layer is aligned iff its xres and yres equal to_grid's and its offsets ox = (e0_k - e0_d) / xres, oy = (n0_d - n0_k) /
    yres (float64) are within 1e-6 cell of integers -- a stated choice: world-file doubles at UTM magnitudes resolve about
    1e-10 cell of 5 m, and 1e-6 cell is 5 micrometres.  An unaligned layer raises ValueError unless align = "nearest" or
    "bilinear", which regrid()s it first onto the part of to_grid's lattice it covers.  The defaults (feather 16, 1e-6 cell)
    are a choice for 5 m grids on a synthetic scene, not tuned on real data.
    -> (to_grid.height, to_grid.width) float32, then with return_count uint8 the number of valid layers per cell, with
    return_source uint8 the layer taken (first .. max) or weighing most (mean: the first valid; feather; 255 = none), with
    return_spread float32 highest - lowest valid layer (the overlap-agreement map; nodata where none), in that order; numpy
    if dsms[0] came as numpy, device tensors otherwise."""
    if mode not in MOSAIC_MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MOSAIC_MODES), mode))
    align = _align_checked(align)
    feather = _int_checked(feather, "feather", 1, MAX_DIST)
    to_grid, dsms, grids, plan = _plan_layers(dsms, grids, to_grid, align)
    dev, as_numpy, layers = _place_layers(dsms, grids, plan, align, nodata)
    gw, gh = int(to_grid.width), int(to_grid.height)
    nd = float(np.float32(nodata))
    d2 = None
    if mode == "feather":
        d2 = [_dist((torch.isfinite(z) & (z != nd)).to(torch.uint8), feather, True) for z, _, _ in layers]
    table = _layer_table(layers, d2)
    out = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    count = torch.empty((gh, gw), dtype=torch.uint8, device=dev) if return_count else None
    source = torch.empty((gh, gw), dtype=torch.uint8, device=dev) if return_source else None
    spread = torch.empty((gh, gw), dtype=torch.float32, device=dev) if return_spread else None
    _call(dev, "smvs_dsm_mosaic", table, len(layers), float(nodata), MOSAIC_MODES[mode], feather, gw, gh, out, count, source, spread)
    del layers, d2                                           # every layer's tensors, alive until the call is enqueued
    return _back(as_numpy, *([out] + [t for t in (count, source, spread) if t is not None]))


# ---- stack fusion: order statistics along the layer axis -----------------------------------------------------------------------
MAX_STACK_LEVELS = 8                                              # levels of one smvs_dsm_stack_select call


def _stack_select(dev, table, n_layers, gw, gh, nodata, fr, centre):
    """smvs_dsm_stack_select over the levels fr in chunks of 8 -> count uint8 (gh, gw), lo, hi float32 (Q, gh, gw).  A chunk without
    a level between two ranks (num % den == 0 throughout) asks for no hi: it is lo."""
    count = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    lo = torch.empty((len(fr), gh, gw), dtype=torch.float32, device=dev)
    hi = torch.empty_like(lo)
    for s0 in range(0, len(fr), MAX_STACK_LEVELS):
        chunk = fr[s0:s0 + MAX_STACK_LEVELS]
        split = any(num % den != 0 for num, den in chunk)
        _call(dev, "smvs_dsm_stack_select", table, n_layers, nodata, np.array(chunk, dtype=np.int32), len(chunk), centre, gw, gh,
              count if s0 == 0 else None, lo[s0:s0 + len(chunk)], hi[s0:s0 + len(chunk)] if split else None)
        if not split:
            hi[s0:s0 + len(chunk)] = lo[s0:s0 + len(chunk)]
    return count, lo, hi


def _stack_quantiles(dev, table, n_layers, gw, gh, nodata, fr, method, centre, min_layers):
    count, lo, hi = _stack_select(dev, table, n_layers, gw, gh, nodata, fr, centre)
    lo_rank, _, rem, den = quantile_ranks(count.reshape(-1).to(torch.int32), fr)
    grids = lambda t: t.t().reshape(lo.shape)                # (cells, Q) -> (Q, gh, gw)
    value = _quantile_value(lo, hi, grids(lo_rank), grids(rem), den[:, None, None], method)
    value = torch.where((count >= max(min_layers, 1))[None], value, torch.full_like(value, float("nan")))
    return count, lo, hi, value


def _stack_inputs(dsms, grids, to_grid, align, min_layers, nodata, centre=None):
    """The checks and the planning the stack functions share, every check before any device work
    -> (dev, as_numpy, layers, table, gw, gh, min_layers, centre on the device or None)."""
    align = _align_checked(align)
    min_layers = _int_checked(min_layers, "min_layers", 0, MAX_MOSAIC_LAYERS)
    to_grid, dsms, grids, plan = _plan_layers(dsms, grids, to_grid, align)
    gw, gh = int(to_grid.width), int(to_grid.height)
    if centre is not None:
        if not isinstance(centre, torch.Tensor):
            centre = np.asarray(centre)
        if tuple(centre.shape) != (gh, gw) or centre.dtype not in (np.float32, torch.float32):
            raise ValueError("centre is float32 of the destination's shape (%d, %d), got %s %s" % (gh, gw, centre.dtype, tuple(centre.shape)))
    dev, as_numpy, layers = _place_layers(dsms, grids, plan, align, nodata)
    if centre is not None:
        centre = _to_device(centre, dev=dev)[0]
    return dev, as_numpy, layers, _layer_table(layers), gw, gh, min_layers, centre


def stack_quantiles(dsms, grids, to_grid=None, q=(0.5,), method="linear", centre=None, align=None, min_layers=1, nodata=-999.0):
    """Exact quantiles, cell by cell, of a stack of DSMs of the same ground (include/satmvs.h smvs_dsm_stack_select, DESIGN.md
    section 9, "Stack fusion"): one per stereo pair, triplet, date or sgm_heights run.  dsms, grids, to_grid and align are
    mosaic()'s, and so is the placing of the layers (at most 64); a layer counts at a cell iff its value there is finite and
    != nodata.  q, method: as in label_quantiles().  With centre ((gh, gw) float32 of the destination) the statistics at cell p
    are those of |z - centre[p]| (float64 difference, rounded to float32 once); a p whose centre is not finite has no layer.
    -> dict: n_valid uint8 (gh, gw), the layers that count; lo, hi float32 (Q, gh, gw), the order statistics of
    quantile_ranks() among them, layer values with their own bits (order: -0.0 below +0.0), nodata where n_valid is 0; value
    float64 (Q, gh, gw) by `method`, NaN where n_valid < max(min_layers, 1).  Selection, no sums: equal bits from run to run.
    numpy if dsms[0] came as numpy, device tensors otherwise."""
    fr = _quantile_fractions(q)
    if method not in QUANTILE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (QUANTILE_METHODS, method))
    dev, as_numpy, layers, table, gw, gh, min_layers, c = _stack_inputs(dsms, grids, to_grid, align, min_layers, nodata, centre)
    count, lo, hi, value = _stack_quantiles(dev, table, len(layers), gw, gh, float(nodata), fr, method, c, min_layers)
    del layers                                               # every layer's tensor, alive until the calls are enqueued
    return {k: _back(as_numpy, t) for k, t in (("n_valid", count), ("lo", lo), ("hi", hi), ("value", value))}


def stack_median(dsms, grids, to_grid=None, align=None, min_layers=1, nodata=-999.0):
    """The per-cell median DSM of a stack: (float) of the "linear" median of stack_quantiles() (for an even number of layers
    lo + (hi - lo) 0.5 in float64), nodata where fewer than max(min_layers, 1) layers count.  Its bits are those of fuse_stack()'s
    `median`.  -> (gh, gw) float32."""
    dev, as_numpy, layers, table, gw, gh, min_layers, _ = _stack_inputs(dsms, grids, to_grid, align, min_layers, nodata)
    count, _, _, value = _stack_quantiles(dev, table, len(layers), gw, gh, float(nodata), [(1, 2)], "linear", None, min_layers)
    del layers
    return _back(as_numpy, _focal_grid(value[0], count >= max(min_layers, 1), nodata))


def stack_nmad(dsms, grids, to_grid=None, align=None, min_layers=1, nodata=-999.0):
    """The robust centre and spread of a stack, cell by cell: focal_nmad()'s two selections along the layer axis.  median float64
    (gh, gw), the linear median of stack_quantiles(); mad, the linear median of |z - float32(median)| over the same layers; nmad =
    1.4826 mad; n_valid uint8.  NaN where n_valid < max(min_layers, 1); (float) of median and mad are fuse_stack()'s `median` and
    `mad`.  -> dict."""
    dev, as_numpy, layers, table, gw, gh, min_layers, _ = _stack_inputs(dsms, grids, to_grid, align, min_layers, nodata)
    nd = float(nodata)
    count, _, _, median = _stack_quantiles(dev, table, len(layers), gw, gh, nd, [(1, 2)], "linear", None, min_layers)
    _, _, _, mad = _stack_quantiles(dev, table, len(layers), gw, gh, nd, [(1, 2)], "linear", median[0].float(), min_layers)
    del layers
    return dict(zip(("median", "mad", "nmad", "n_valid"), _back(as_numpy, median[0], mad[0], mad[0] * NMAD_FACTOR, count)))


def fuse_stack(dsms, grids, to_grid=None, k=3.0, floor=0.5, min_layers=1, align=None, nodata=-999.0, return_info=False):
    """A stack of DSMs of the same ground fused robustly, cell by cell (include/satmvs.h smvs_dsm_stack_fuse, DESIGN.md section 9,
    "Stack fusion"): the mean (float64, in the list's order) of the layers within max(k nmad, floor) of the stack's median there,
    nmad = 1.4826 mad, the median and the MAD those of stack_nmad() -- despike_robust()'s rule along the layer axis, so one cloud,
    one mismatched pair or one new building does not move the cell.  dsms, grids, to_grid and align are mosaic()'s (at most 64
    layers).  A cell with fewer than max(min_layers, 1) layers gets nodata; where no layer passes (an even number of layers, two
    different middle values and a small k and floor) the cell gets the median; one layer alone comes back bit for bit.  The
    threshold's factor k 1.4826 is formed here in float64.  The defaults (k 3, floor 0.5 m) are despike_robust()'s, chosen on a
    synthetic scene and not tuned on real data.
    -> (gh, gw) float32, and with return_info a dict beside it: median, mad float32; count, n_inliers uint8; members, inliers
    int64 with bit j set where layer j counts / is an inlier (stack_outliers() reads them).  numpy if dsms[0] came as numpy."""
    k, floor = _finite(k, "k"), _finite(floor, "floor")
    if k < 0.0 or floor < 0.0:
        raise ValueError("k and floor must be >= 0, got %r and %r" % (k, floor))
    dev, as_numpy, layers, table, gw, gh, min_layers, _ = _stack_inputs(dsms, grids, to_grid, align, min_layers, nodata)
    out = torch.empty((gh, gw), dtype=torch.float32, device=dev)
    info = {}
    if return_info:
        for name, dtype in (("median", torch.float32), ("mad", torch.float32), ("count", torch.uint8), ("n_inliers", torch.uint8),
                            ("members", torch.int64), ("inliers", torch.int64)):
            info[name] = torch.empty((gh, gw), dtype=dtype, device=dev)
    _call(dev, "smvs_dsm_stack_fuse", table, len(layers), float(nodata), k * NMAD_FACTOR, floor, min_layers, gw, gh, out,
          *[info.get(name) for name in ("median", "mad", "count", "n_inliers", "members", "inliers")])
    del layers
    if not return_info:
        return _back(as_numpy, out)
    return _back(as_numpy, out), {name: _back(as_numpy, t) for name, t in info.items()}


def stack_outliers(info, k):
    """Where layer k of a fused stack disagrees with the consensus: 1 where it counts at the cell but is no inlier (a cloud, a
    change, a mismatch), from the `members` and `inliers` of fuse_stack(..., return_info=True).  -> (gh, gw) uint8, of info's kind."""
    k = _int_checked(k, "k", 0, MAX_MOSAIC_LAYERS - 1)
    members, inliers = info["members"], info["inliers"]
    if isinstance(members, torch.Tensor):
        return (((members & ~inliers) >> k) & 1).to(torch.uint8)
    return ((np.asarray(members) & ~np.asarray(inliers)) >> np.int64(k) & np.int64(1)).astype(np.uint8)


# ---- orthophoto ---------------------------------------------------------------------------------------------------------------
ORTHO_STATES = ("no height", "outside", "occluded", "visible")     # the state codes 0 .. 3 of visibility() / smvs_rpc_ortho
MAX_CHANNELS = 16


def _occ_tol_checked(occ_tol):
    t = float(occ_tol)
    if not (math.isfinite(t) and t >= 0.0):
        raise ValueError("occ_tol must be finite and >= 0, got %r" % t)
    return t


def _ortho_call(z, grid, nodata, tm7, r, image, H, W, C, x0, y0, h_hi, occlusion, occ_tol, view, ortho, source, state):
    _call(z.device, "smvs_rpc_ortho", z, grid.width, grid.height, grid.grid4(), float(nodata), tm7, r, image, H, W, C, x0, y0,
          h_hi, 1 if occlusion else 0, occ_tol, view, ortho, source, state)


def visibility(dsm, grid, rpc, projection, shape, origin=(0, 0), nodata=-999.0, occlusion=True, occ_tol=0.5):
    """What one view sees of every DSM cell (include/satmvs.h smvs_rpc_ortho for the exact definition):
    (gh, gw) uint8 with 0 = no height (nodata or non-finite cell), 1 = the cell projects outside the (H, W) = `shape` tile whose
    upper-left pixel is `origin` = (x0, y0), 2 = occluded (the ray from the cell towards the sensor passes more than occ_tol [m]
    under the bilinear DSM surface; only with occlusion=True), 3 = visible.  The top of the march, h_hi, is the highest valid
    cell.  Numpy if the DSM came as numpy, a device tensor otherwise."""
    H, W, x0, y0 = _tile(shape, origin)
    occ_tol = _occ_tol_checked(occ_tol)
    dsm = _dsm_converted(dsm, grid)
    r = _rpc_checked(rpc)
    dev = _dev()
    z, as_numpy = _to_device(dsm, torch.float32, dev)
    r, _ = _to_device(r, torch.float64, dev)
    _, h_hi = _valid_range(z, nodata, lower=False)
    state = torch.empty((grid.height, grid.width), dtype=torch.uint8, device=dev)
    _ortho_call(z, grid, nodata, projection.tm7(), r, None, H, W, 1, x0, y0, h_hi, occlusion, occ_tol, 0, None, None, state)
    return _back(as_numpy, state)


def _images_checked(images):
    """[(H, W, C) arrays or tensors of a real dtype] of one image or a list; every view has the same C, 1 <= C <= 16."""
    ims = list(images) if isinstance(images, (list, tuple)) else [images]
    if not ims:
        raise ValueError("no image")
    out = []
    for im in ims:
        if not isinstance(im, torch.Tensor):
            im = np.asarray(im)
            if not (np.issubdtype(im.dtype, np.integer) or np.issubdtype(im.dtype, np.floating) or im.dtype == np.bool_):
                raise ValueError("images must have a real dtype, got %s" % im.dtype)
        elif im.is_complex():
            raise ValueError("images must have a real dtype, got %s" % im.dtype)
        if im.ndim == 2:
            im = im[:, :, None]
        if im.ndim != 3:
            raise ValueError("images are (H, W) or (H, W, C), got %s" % (tuple(im.shape),))
        if not 1 <= im.shape[2] <= MAX_CHANNELS:
            raise ValueError("images must have 1 .. %d channels, got %d" % (MAX_CHANNELS, im.shape[2]))
        out.append(im)
    if len({im.shape[2] for im in out}) != 1:
        raise ValueError("every view must have the same number of channels, got %s" % [im.shape[2] for im in out])
    return out


def _order_checked(order, n):
    if isinstance(order, str):
        if order not in ("nadir", "given"):
            raise ValueError('order must be "nadir", "given" or a permutation of the view indices, got %r' % order)
        return order
    try:
        seq = [int(i) for i in order]
        ok = all(isinstance(i, (int, np.integer)) and not isinstance(i, bool) for i in order)
    except (TypeError, ValueError):
        seq, ok = [], False
    if not ok or sorted(seq) != list(range(n)):
        raise ValueError("order must be \"nadir\", \"given\" or a permutation of range(%d), got %r" % (n, order))
    return seq


def nadir_order(rpcs, grid, projection, h_top):
    """View indices from the most to the least nadir: by the mean ground shift per metre of height, |G(h_top) - G(h_top - 100)|
    / 100 m with G(h) = TM_forward(photo2obj(x, y, h)), at the grid's centre and the four points a quarter of the grid away from
    it along the axes, (x, y) being each point's pixel at h_top - 100.  Ties go by index.  Host float64 RPCs (rpc_synth) and the
    device TM (projection.proj)."""
    from . import rpc_synth
    ec = grid.e0 + 0.5 * (grid.width - 1) * grid.xres
    nc = grid.n0 - 0.5 * (grid.height - 1) * grid.yres
    qe, qn = 0.25 * grid.width * grid.xres, 0.25 * grid.height * grid.yres
    en = np.array([[ec, nc], [ec - qe, nc], [ec + qe, nc], [ec, nc - qn], [ec, nc + qn]], np.float64)
    ll = projection.proj(en, reverse=True)
    h0, h1 = h_top - 100.0, h_top
    pts = []
    for rpc in rpcs:
        rpc = np.asarray(torch.as_tensor(rpc).detach().cpu(), np.float64).reshape(-1)
        x, y = rpc_synth.obj2photo(rpc, ll[:, 0], ll[:, 1], np.full(len(ll), h0))
        for h in (h0, h1):
            lat, lon = rpc_synth.photo2obj(rpc, x, y, np.full(len(ll), h))
            pts.append(np.stack([lat, lon], -1))
    g = projection.proj(np.stack(pts)).reshape(len(rpcs), 2, len(ll), 2)
    shift = np.hypot(g[:, 1, :, 0] - g[:, 0, :, 0], g[:, 1, :, 1] - g[:, 0, :, 1]).mean(axis=1) / (h1 - h0)
    return sorted(range(len(rpcs)), key=lambda i: (shift[i], i))


def orthorectify(images, rpcs, dsm, grid, projection, origins=None, nodata=-999.0, occlusion=True, occ_tol=0.5, order="nadir",
                 fill=float("nan"), return_source=False):
    """A true orthophoto: the views' images resampled onto the DSM's grid, each cell from the first view, in `order`, that sees
    it (visibility() state 3), bilinearly (pixel centres on integers); cells no view sees keep `fill`.  images: one image or a
    list, each (H, W) or (H, W, C) of any real dtype (taken as float32), the same C <= 16 for all; rpcs: one 170-vector per
    view; origins: the (x0, y0) of each image in its view (None: all (0, 0)).  order: "nadir" (nadir_order: the least ground
    shift per metre of height first), "given", or a permutation of the view indices.  No blending between views.
    -> (gh, gw, C) float32 and, with return_source, (gh, gw) int32 = the index of the view in `images` that filled each cell
    (-1: none); numpy if the DSM came as numpy, device tensors otherwise."""
    ims = _images_checked(images)
    n = len(ims)
    rs = _rpc_list(rpcs)
    if len(rs) != n:
        raise ValueError("one RPC per image: %d images, %d rpcs" % (n, len(rs)))
    rs = [_rpc_checked(r) for r in rs]
    if origins is None:
        origins = [(0, 0)] * n
    elif n == 1 and len(origins) == 2 and all(isinstance(t, (int, np.integer)) for t in origins):
        origins = [origins]
    if len(origins) != n:
        raise ValueError("one origin per image: %d images, %d origins" % (n, len(origins)))
    tiles = [_tile(im.shape[:2], o) for im, o in zip(ims, origins)]
    occ_tol = _occ_tol_checked(occ_tol)
    seq = _order_checked(order, n)
    fill = float(fill)
    dsm = _dsm_converted(dsm, grid)
    dev = _dev()
    z, as_numpy = _to_device(dsm, torch.float32, dev)
    _, h_hi = _valid_range(z, nodata, lower=False)
    if seq == "given":
        seq = list(range(n))
    elif seq == "nadir":
        seq = nadir_order(rs, grid, projection, h_hi)
    C = int(ims[0].shape[2])
    ortho = torch.full((grid.height, grid.width, C), fill, dtype=torch.float32, device=dev)
    source = torch.full((grid.height, grid.width), -1, dtype=torch.int32, device=dev)
    tm7 = projection.tm7()
    for v in seq:
        im, _ = _to_device(ims[v], torch.float32, dev)
        r, _ = _to_device(rs[v], torch.float64, dev)
        H, W, x0, y0 = tiles[v]
        _ortho_call(z, grid, nodata, tm7, r, im, H, W, C, x0, y0, h_hi, occlusion, occ_tol, v, ortho, source, None)
    ortho, source = _back(as_numpy, ortho, source)
    return (ortho, source) if return_source else ortho


def _write_tfw(path, grid):
    text = str(grid.xres) + "\n0\n0\n" + str(-grid.yres) + "\n" + str(grid.e0) + "\n" + str(grid.n0)
    with open(os.path.splitext(path)[0] + ".tfw", "w") as f:
        f.write(text)


def write_ortho(path, ortho, grid):
    """An orthophoto as a TIFF (Pillow) plus the world file (.tfw) of write_dsm: uint8 (gh, gw), (gh, gw, 1) or (gh, gw, 3) as
    L or RGB, float32 (gh, gw) or (gh, gw, 1) as F.  Anything else raises ValueError (convert first, e.g.
    np.nan_to_num(o).clip(0, 255).astype(np.uint8))."""
    from PIL import Image
    a = ortho.detach().cpu().numpy() if isinstance(ortho, torch.Tensor) else np.asarray(ortho)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[:2] != (grid.height, grid.width):
        raise ValueError("ortho shape %s differs from the grid's (%d, %d[, C])" % (a.shape, grid.height, grid.width))
    C = a.shape[2]
    if not ((a.dtype == np.uint8 and C in (1, 3)) or (a.dtype == np.float32 and C == 1)):
        raise ValueError("write_ortho writes uint8 with 1 or 3 channels or float32 with 1, got %s with %d" % (a.dtype, C))
    Image.fromarray(np.ascontiguousarray(a[:, :, 0] if C == 1 else a)).save(path, format="TIFF")
    _write_tfw(path, grid)
    return path


def write_dsm(path, dsm, grid):
    """A float32 TIFF (Pillow) and, beside it, the world file (.tfw) in the six-line form of the reference's
    gdal_create_dsm_file (dataset/data_io.py:289-296): xres, 0, 0, -yres, E and N of the centre of the upper-left cell."""
    from PIL import Image
    a = dsm.detach().cpu().numpy() if isinstance(dsm, torch.Tensor) else np.asarray(dsm)
    a = np.ascontiguousarray(a, dtype=np.float32)
    _on_grid(a, grid)
    Image.fromarray(a, mode="F").save(path, format="TIFF")
    _write_tfw(path, grid)
    return path


def read_dsm(path):
    """(dsm float32, DSMGrid) of a TIFF written by write_dsm (or any float32 TIFF with a north-up .tfw beside it)."""
    from PIL import Image
    from .data_io import read_tfw
    a = np.array(Image.open(path), dtype=np.float32)
    t = read_tfw(os.path.splitext(path)[0] + ".tfw")
    if t[1] != 0.0 or t[2] != 0.0:
        raise ValueError("rotated world files are not supported")
    return a, DSMGrid(float(t[4]), float(t[5]), float(t[0]), float(-t[3]), a.shape[1], a.shape[0])


def dsm_metrics(est, gt, nodata, thresholds=(2.5, 7.5)):
    """Accuracy of a DSM against a ground-truth DSM on the same grid (float64).  Cells equal to `nodata` or non-finite are
    invalid.  -> dict: mae, rmse (over cells valid in both), "<t" = share of those cells with |est - gt| < t per threshold,
    completeness = share of valid ground-truth cells that have an estimate, n = number of cells compared."""
    e = torch.as_tensor(est).to(torch.float64)
    g = torch.as_tensor(gt).to(device=e.device, dtype=torch.float64)
    if e.shape != g.shape:
        raise ValueError("shapes differ: %s vs %s" % (tuple(e.shape), tuple(g.shape)))
    vg = torch.isfinite(g) & (g != nodata)
    ve = torch.isfinite(e) & (e != nodata)
    both = vg & ve
    nb, ng = int(both.sum()), int(vg.sum())
    out = {"n": nb, "completeness": nb / ng if ng else float("nan")}
    if nb:
        d = (e[both] - g[both]).abs()
        out["mae"] = float(d.mean())
        out["rmse"] = float(torch.sqrt((d * d).mean()))
        for t in thresholds:
            out["<%g" % t] = float((d < t).double().mean())
    else:
        out["mae"] = out["rmse"] = float("nan")
        for t in thresholds:
            out["<%g" % t] = float("nan")
    return out


def dsm_metrics_robust(est, gt, nodata=-999.0, levels=(0.6827, 0.9, 0.95)):
    """The accuracy figures that survive outliers, on the device: est and gt on the same grid (any real dtype, taken as
    float32), a cell compared iff both are finite and != nodata; d = (float)((double)est - (double)gt) there, one zone over
    the grid, label_quantiles() and label_nmad() on it (so exact order statistics, equal bits from run to run).
    -> dict of Python numbers: n = the cells compared; median = the linear median of d; nmad = 1.4826 x the linear median of
    |d - float32(median)|; "le68", "le90", "le95" (a level's key is its rounded percentage) = the linear quantile of |d| at
    that level.  NaN where n is 0.  A d that is not finite in float32 is not compared.  Reading the figures is the one
    synchronisation."""
    fr = _quantile_fractions(levels)
    e, _ = _to_device(est if isinstance(est, torch.Tensor) else np.asarray(est), torch.float32)
    g, _ = _to_device(gt if isinstance(gt, torch.Tensor) else np.asarray(gt), torch.float32, e.device)
    if e.ndim != 2 or e.shape != g.shape:
        raise ValueError("est and gt are (gh, gw) grids of one shape, got %s and %s" % (tuple(e.shape), tuple(g.shape)))
    nd = float(np.float32(nodata))
    both = torch.isfinite(e) & (e != nd) & torch.isfinite(g) & (g != nd)
    d = (e.double() - g.double()).float()
    zone = both.to(torch.int32)
    nan = float("nan")                                       # the zone map says which cells count: no value of d is set aside
    spread = label_nmad(zone, 1, d, nodata=nan)
    le = label_quantiles(zone, 1, d, fr, "linear", torch.zeros(1, dtype=torch.float32, device=e.device), nan)
    out = {"n": int(spread["n_valid"][0]), "median": float(spread["median"][0]), "nmad": float(spread["nmad"][0])}
    for (num, den), v in zip(fr, le["value"][0].tolist()):
        out["le%d" % ((200 * num + den) // (2 * den))] = v
    return out


# ---- the sun: cast shadows, gradient, shaded relief, exposure -------------------------------------------------------------------
def _sun_checked(azimuth, elevation):
    azimuth, elevation = float(azimuth), float(elevation)
    if not math.isfinite(azimuth):
        raise ValueError("azimuth must be finite [degrees clockwise from north], got %r" % azimuth)
    if not 0.0 < elevation < 90.0:
        raise ValueError("elevation must be above 0 and below 90 degrees, got %r" % elevation)
    return azimuth, elevation


def _shadow_tol_checked(tol):
    tol = float(tol)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0, got %r" % tol)
    return tol


def sun_terms(grid, azimuth, elevation):
    """The four doubles smvs_dsm_shadow takes for a sun at `azimuth` [degrees clockwise from north, TOWARDS the sun, any finite
    value] and `elevation` [degrees, above 0 and below 90] over `grid`: with sA, cA = sin, cos(radians(azimuth)) and k =
    tan(radians(elevation)), ucol = sA / xres, urow = -cA / yres (the direction towards the sun in cells; rows run south),
    a = k xres sA, b = -k yres cA (k times the distance towards the sun, per column and per row).  -> (ucol, urow, a, b)."""
    azimuth, elevation = _sun_checked(azimuth, elevation)
    _grid_checked(grid, "grid")
    xres, yres = float(grid.xres), float(grid.yres)
    sA, cA = math.sin(math.radians(azimuth)), math.cos(math.radians(azimuth))
    k = math.tan(math.radians(elevation))
    return sA / xres, -cA / yres, k * xres * sA, -k * yres * cA


def _shadow_workspace(z):
    gh, gw = z.shape
    nbytes = _lib.load().smvs_dsm_shadow_workspace_bytes(gw, gh)
    if nbytes == 0:
        raise ValueError("unsupported shadow casting: %d x %d cells" % (gw, gh))
    return torch.empty(nbytes, dtype=torch.uint8, device=z.device), nbytes


def _shadow(z, terms, nodata, tol, ws, nbytes, want_depth=False):
    """smvs_dsm_shadow on a device grid with a workspace the caller keeps -> (shade, depth or None)."""
    gh, gw = z.shape
    shade = torch.empty((gh, gw), dtype=torch.uint8, device=z.device)
    depth = torch.empty((gh, gw), dtype=torch.float32, device=z.device) if want_depth else None
    _call(z.device, "smvs_dsm_shadow", z, gw, gh, float(nodata), *terms, tol, shade, depth, ws, nbytes)
    return shade, depth


def cast_shadows(dsm, grid, azimuth, elevation, nodata=-999.0, tol=0.1, return_depth=False):
    """The cells of a DSM in cast shadow for one sun (include/satmvs.h smvs_dsm_shadow, DESIGN.md section 9, "Sun").  azimuth:
    degrees clockwise from north TOWARDS the sun, any finite value; 0 < elevation < 90 degrees.  Along a line of cells that
    runs towards the sun, a cell is shadowed iff the highest g = z - tan(elevation) (distance towards the sun) among the valid
    cells sunward of it exceeds its own g by more than tol [m]; the lines are the grid's rows or columns sheared by whole
    cells, within less than a cell of the true ray, and the reach is unbounded.  Invalid cells neither cast nor receive.
    The default tol (0.1 m) is a choice for 5 m grids, not tuned on real data: it keeps float32 rounding of the
    heights from shading a plane that runs exactly along the ray.  dsm (grid.height, grid.width) of any real dtype (taken as
    float32), numpy or a device tensor.
    -> shade (gh, gw) uint8: 0 invalid, 1 lit, 2 shadowed (and, with return_depth, depth (gh, gw) float32: how far [m] the
    cell lies under the shadow line, negative where lit, -inf where nothing lies sunward, nodata at invalid cells); numpy if
    the DSM came as numpy, device tensors otherwise."""
    terms = sun_terms(grid, azimuth, elevation)
    tol = _shadow_tol_checked(tol)
    dsm = _dsm_converted(dsm, grid)
    z, as_numpy = _to_device(dsm, torch.float32)
    ws, nbytes = _shadow_workspace(z)
    shade, depth = _shadow(z, terms, nodata, tol, ws, nbytes, return_depth)
    shade, depth = _back(as_numpy, shade, depth)
    return (shade, depth) if return_depth else shade


def _gradient(z, grid, nodata):
    gh, gw = z.shape
    dzde, dzdn = torch.empty_like(z), torch.empty_like(z)
    _call(z.device, "smvs_dsm_gradient", z, gw, gh, float(nodata), float(grid.xres), float(grid.yres), dzde, dzdn)
    return dzde, dzdn


def _relief_input(dsm, grid):
    _grid_checked(grid, "grid")
    return _to_device(_dsm_converted(dsm, grid), torch.float32)


def gradient(dsm, grid, nodata=-999.0):
    """Horn's 3 x 3 gradient of a DSM (include/satmvs.h smvs_dsm_gradient): dzde [m/m] towards the east, dzdn towards the
    north; a neighbour off the grid or invalid takes the centre's value; invalid cells get nodata in both.
    -> (dzde, dzdn) (gh, gw) float32; numpy if the DSM came as numpy, device tensors otherwise."""
    z, as_numpy = _relief_input(dsm, grid)
    return _back(as_numpy, *_gradient(z, grid, nodata))


def _valid_cells(z, nodata):
    return torch.isfinite(z) & (z != float(np.float32(nodata)))


def slope(dsm, grid, nodata=-999.0, degrees=True):
    """The steepest slope atan(sqrt(dzde^2 + dzdn^2)) of gradient(), float64 element-wise, in degrees or radians; NaN at
    invalid cells.  -> (gh, gw) float32."""
    z, as_numpy = _relief_input(dsm, grid)
    dzde, dzdn = (t.double() for t in _gradient(z, grid, nodata))
    s = torch.atan(torch.sqrt(dzde * dzde + dzdn * dzdn))
    if degrees:
        s = torch.rad2deg(s)
    return _back(as_numpy, torch.where(_valid_cells(z, nodata), s, torch.full_like(s, float("nan"))).float())


def aspect(dsm, grid, nodata=-999.0):
    """The downslope azimuth atan2(-dzde, -dzdn) of gradient() in degrees clockwise from north, in [0, 360); NaN on flat
    cells (both components 0) and at invalid cells.  -> (gh, gw) float32."""
    z, as_numpy = _relief_input(dsm, grid)
    dzde, dzdn = (t.double() for t in _gradient(z, grid, nodata))
    a = torch.rad2deg(torch.atan2(-dzde, -dzdn))
    a = torch.where(a < 0.0, a + 360.0, a).float()
    a = torch.where(a >= 360.0, torch.zeros_like(a), a)      # -1e-12 + 360 rounds to 360 in float32
    flat = (dzde == 0.0) & (dzdn == 0.0)
    return _back(as_numpy, torch.where(_valid_cells(z, nodata) & ~flat, a, torch.full_like(a, float("nan"))))


def _cos_incidence(dzde, dzdn, azimuth, elevation):
    """max(0, (sinE - cosE (dzde sA + dzdn cA)) / sqrt(1 + dzde^2 + dzdn^2)) in float64, the operations in this order."""
    sA, cA = math.sin(math.radians(azimuth)), math.cos(math.radians(azimuth))
    sE, cE = math.sin(math.radians(elevation)), math.cos(math.radians(elevation))
    num = sE - cE * (dzde * sA + dzdn * cA)
    return torch.clamp(num / torch.sqrt(1.0 + dzde * dzde + dzdn * dzdn), min=0.0)


def hillshade(dsm, grid, azimuth=315.0, elevation=45.0, shadows=False, nodata=-999.0, tol=0.1):
    """Shaded relief: the cosine of the sun's incidence on the surface of gradient(), cos i = (sinE - cosE (dzde sA + dzdn
    cA)) / sqrt(1 + dzde^2 + dzdn^2) in float64, clipped at 0; with `shadows`, 0 where cast_shadows(..., tol) says shadowed.
    azimuth, elevation and tol as in cast_shadows (the default sun, north-west at 45 degrees, is the cartographic habit).
    -> (gh, gw) float32 in [0, 1], NaN at invalid cells; numpy if the DSM came as numpy, a device tensor otherwise."""
    azimuth, elevation = _sun_checked(azimuth, elevation)
    tol = _shadow_tol_checked(tol)
    terms = sun_terms(grid, azimuth, elevation) if shadows else None
    z, as_numpy = _relief_input(dsm, grid)
    dzde, dzdn = (t.double() for t in _gradient(z, grid, nodata))
    h = _cos_incidence(dzde, dzdn, azimuth, elevation)
    if shadows:
        ws, nbytes = _shadow_workspace(z)
        shade, _ = _shadow(z, terms, nodata, tol, ws, nbytes)
        h = torch.where(shade == 2, torch.zeros_like(h), h)
    return _back(as_numpy, torch.where(_valid_cells(z, nodata), h, torch.full_like(h, float("nan"))).float())


def sun_exposure(dsm, grid, suns, weights=None, incidence=True, nodata=-999.0, tol=0.1):
    """What a list of suns leaves on every cell: the float64 sum, in the list's order, of w lit (cos i if incidence else 1),
    lit = 1 where cast_shadows does not say shadowed, cos i as in hillshade.  suns: a list of (azimuth, elevation) pairs, e.g.
    the sun's positions through a day; weights: one finite number per sun (None: all 1), e.g. hours or irradiance.  One
    workspace serves the whole list (its size depends on the grid alone).  With the labels of extract_objects,
    label_stats(labels, n, values=exposure)["mean"] is the sun each roof gets.
    -> (gh, gw) float32, NaN at invalid cells; numpy if the DSM came as numpy, a device tensor otherwise."""
    try:
        suns = [_sun_checked(*s) for s in suns]
    except TypeError:
        raise ValueError("suns must be a list of (azimuth, elevation) pairs, got %r" % (suns,)) from None
    if not suns:
        raise ValueError("sun_exposure needs at least one sun")
    weights = [1.0] * len(suns) if weights is None else [_finite(w, "a weight") for w in weights]
    if len(weights) != len(suns):
        raise ValueError("one weight per sun: %d suns, %d weights" % (len(suns), len(weights)))
    tol = _shadow_tol_checked(tol)
    terms = [sun_terms(grid, az, el) for az, el in suns]
    z, as_numpy = _relief_input(dsm, grid)
    ws, nbytes = _shadow_workspace(z)
    total = torch.zeros(z.shape, dtype=torch.float64, device=z.device)
    if incidence:
        dzde, dzdn = (t.double() for t in _gradient(z, grid, nodata))
    for (az, el), w, t in zip(suns, weights, terms):
        shade, _ = _shadow(z, t, nodata, tol, ws, nbytes)
        term = _cos_incidence(dzde, dzdn, az, el) * w if incidence else torch.full_like(total, w)
        total = total + torch.where(shade == 2, torch.zeros_like(term), term)
    return _back(as_numpy, torch.where(_valid_cells(z, nodata), total, torch.full_like(total, float("nan"))).float())


# ---- horizon maps: tangents towards a list of azimuths, sky view, any-sun visibility ---------------------------------------------
MAX_HORIZON_DIRS = 64                                             # directions of one smvs_dsm_horizon call
HORIZON_INTERP = ("linear", "nearest")


def _azimuths_checked(azimuths):
    try:
        out = [float(a) for a in azimuths]
    except TypeError:
        raise ValueError("azimuths must be a list of numbers [degrees clockwise from north], got %r" % (azimuths,)) from None
    if not out:
        raise ValueError("at least one azimuth is needed")
    for a in out:
        if not math.isfinite(a):
            raise ValueError("azimuth must be finite [degrees clockwise from north], got %r" % a)
    return out


def horizon_terms(grid, azimuth):
    """The four doubles smvs_dsm_horizon takes for `azimuth` [degrees clockwise from north, any finite value] over `grid`: with
    sA, cA = sin, cos(radians(azimuth)), ucol = sA / xres, urow = -cA / yres (the direction towards the azimuth in cells; rows
    run south), a = 256 xres sA, b = -256 yres cA (the position along the azimuth in units of 2^-8 m, per column and per row).
    -> (ucol, urow, a, b)."""
    azimuth = _finite(azimuth, "azimuth")
    _grid_checked(grid, "grid")
    xres, yres = float(grid.xres), float(grid.yres)
    sA, cA = math.sin(math.radians(azimuth)), math.cos(math.radians(azimuth))
    return sA / xres, -cA / yres, 256.0 * xres * sA, -256.0 * yres * cA


def horizon_azimuths(n):
    """n evenly spaced azimuths [degrees] starting at 0 (north), clockwise."""
    n = _int_checked(n, "n", 1, 1 << 20)
    return [360.0 * i / n for i in range(n)]


def _horizon_dirs(grid, azimuths):
    """(K, 4) float64 host array of horizon_terms, checked against the limits of smvs_dsm_horizon before any device work."""
    dirs = np.array([horizon_terms(grid, a) for a in azimuths], dtype=np.float64).reshape(-1, 4)
    for az, (ucol, urow, a, b) in zip(azimuths, dirs):
        if (abs(b) if abs(urow) >= abs(ucol) else abs(a)) < 4.0:
            raise ValueError("the grid's resolution is too fine for a horizon towards %r: cells below 1/64 m" % az)
        if not abs(a) * grid.width + abs(b) * grid.height < 2.0 ** 37:
            raise ValueError("the grid is too long for a horizon towards %r: its extent must stay below 2^29 m" % az)
    return dirs


def horizon(dsm, grid, azimuths, nodata=-999.0):
    """Horizon maps of a DSM (include/satmvs.h smvs_dsm_horizon, DESIGN.md section 9, "Horizon"): for every azimuth of the list
    [degrees clockwise from north, any finite values, at least one] and every cell, the tangent of the elevation angle of the
    highest thing that stands towards the azimuth, along the same sheared lines of cells as cast_shadows, with unbounded reach:
    the maximum of (z_j - z) / (distance towards the azimuth) over the valid cells j of the line that lie towards it, heights
    and distances in units of 2^-8 m, exact.  -inf where nothing stands towards the azimuth, NaN at invalid cells (not finite,
    nodata, or beyond +-32768 m).  More than 64 azimuths go in chunks of 64; the bits do not depend on the chunking.  dsm
    (grid.height, grid.width) of any real dtype (taken as float32), numpy or a device tensor.
    -> (K, gh, gw) float32; numpy if the DSM came as numpy, a device tensor otherwise."""
    azimuths = _azimuths_checked(azimuths)
    dirs = _horizon_dirs(grid, azimuths)
    dsm = _dsm_converted(dsm, grid)
    z, as_numpy = _to_device(dsm, torch.float32)
    gh, gw = z.shape
    K = len(azimuths)
    nbytes = _lib.load().smvs_dsm_horizon_workspace_bytes(gw, gh, min(K, MAX_HORIZON_DIRS))
    if nbytes == 0:
        raise ValueError("unsupported horizon: %d x %d cells" % (gw, gh))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    out = torch.empty((K, gh, gw), dtype=torch.float32, device=z.device)
    for k0 in range(0, K, MAX_HORIZON_DIRS):
        n = min(MAX_HORIZON_DIRS, K - k0)
        _call(z.device, "smvs_dsm_horizon", z, gw, gh, float(nodata), np.ascontiguousarray(dirs[k0:k0 + n]), n, out[k0:k0 + n], ws, nbytes)
    return _back(as_numpy, out)


def _tan_h_checked(tan_h, azimuths=None):
    """(K, gh, gw) float32 maps as a tensor where they are (numpy: on the host), and whether they came as numpy."""
    as_numpy = not isinstance(tan_h, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(tan_h)) if as_numpy else tan_h
    if t.ndim != 3 or t.shape[0] < 1 or t.dtype != torch.float32:
        raise ValueError("tan_h is (K, gh, gw) float32 with K >= 1, got %s of shape %s" % (t.dtype, tuple(t.shape)))
    if azimuths is not None and len(azimuths) != t.shape[0]:
        raise ValueError("one azimuth per horizon map: %d azimuths, %d maps" % (len(azimuths), t.shape[0]))
    return t, as_numpy


def sky_view_factor(tan_h):
    """The isotropic sky-view factor of a horizontal surface from horizon maps: the float64 mean, in the list's order, of
    1 / (1 + max(t, 0)^2), which is cos^2 of the horizon angle clamped at the horizontal.  1 under an open horizon, NaN at
    invalid cells.  -> (gh, gw) float64, numpy or tensor as tan_h came."""
    t, as_numpy = _tan_h_checked(tan_h)
    total = torch.zeros(t.shape[1:], dtype=torch.float64, device=t.device)
    for k in range(t.shape[0]):
        x = torch.clamp(t[k].double(), min=0.0)
        total = total + 1.0 / (1.0 + x * x)
    svf = total / float(t.shape[0])
    svf = torch.where(torch.isnan(t).any(dim=0), torch.full_like(svf, float("nan")), svf)
    return svf.numpy() if as_numpy else svf


def _horizon_bracket(azimuths, azimuth, interp):
    """[(index, weight)] of the listed azimuths an asked one takes its tangent from: itself (the first listed, weight None)
    if it is in the list modulo 360; else, for "linear", the nearest listed one below and the nearest above around the circle
    with weights 1 - w and w, w = (asked - below) / (above - below); for "nearest", the one at the least distance around the
    circle (the earlier of two at equal distance)."""
    mods = [a % 360.0 for a in azimuths]
    x = azimuth % 360.0
    if x in mods:
        return [(mods.index(x), None)]
    if interp == "nearest":
        dist = [abs((m - x + 180.0) % 360.0 - 180.0) for m in mods]
        return [(dist.index(min(dist)), None)]
    below = [(m, i) for i, m in enumerate(mods) if m < x] or [(max(mods) - 360.0, mods.index(max(mods)))]
    above = [(m, i) for i, m in enumerate(mods) if m > x] or [(min(mods) + 360.0, mods.index(min(mods)))]
    (lo, i), (hi, j) = max(below, key=lambda p: (p[0], -p[1])), min(above)
    w = (x - lo) / (hi - lo)
    return [(i, 1.0 - w), (j, w)]


def _interp_checked(interp):
    if interp not in HORIZON_INTERP:
        raise ValueError("interp must be one of %s, got %r" % (HORIZON_INTERP, interp))
    return interp


def _horizon_tangent(t, azimuths, azimuth, interp):
    """The float64 tangent towards `azimuth` from checked maps, as _horizon_bracket says (NaN at invalid cells)."""
    pick = _horizon_bracket(azimuths, azimuth, interp)
    if len(pick) == 1:
        return t[pick[0][0]].double()
    (i, wi), (j, wj) = pick
    return wi * t[i].double() + wj * t[j].double()


def _horizon_lit(t, azimuths, azimuth, elevation, interp):
    """horizon_lit on a checked tensor -> uint8 tensor."""
    hidden = _horizon_tangent(t, azimuths, azimuth, interp) > math.tan(math.radians(elevation))
    code = torch.where(hidden, 2, 1).to(torch.uint8)
    return torch.where(torch.isnan(t[0]), torch.zeros_like(code), code)


def horizon_lit(tan_h, azimuths, azimuth, elevation, interp="linear"):
    """Whether a source at `azimuth` [degrees clockwise from north, any finite value] and 0 < `elevation` < 90 degrees (the
    sun, a satellite) sees each cell, from the horizon maps tan_h of the listed `azimuths`: a cell is hidden iff T >
    tan(elevation), T = (1 - w) T_below + w T_above in float64 between the two listed azimuths that bracket the asked one around
    the circle (w the asked azimuth's share of the way), or with interp="nearest" the map of the nearest listed azimuth; an
    asked azimuth that is in the list (modulo 360) takes that direction's own map bit for bit.
    -> (gh, gw) uint8 with the codes of cast_shadows: 0 invalid, 1 lit, 2 hidden; numpy or tensor as tan_h came."""
    azimuths = _azimuths_checked(azimuths)
    azimuth, elevation = _sun_checked(azimuth, elevation)
    _interp_checked(interp)
    t, as_numpy = _tan_h_checked(tan_h, azimuths)
    code = _horizon_lit(t, azimuths, azimuth, elevation, interp)
    return code.numpy() if as_numpy else code


def sun_exposure_from_horizon(dsm, grid, tan_h, azimuths, suns, weights=None, incidence=True, nodata=-999.0, interp="linear"):
    """sun_exposure with every sun's `lit` taken from horizon_lit(tan_h, azimuths, ...) instead of a pass of cast_shadows: the
    float64 sum, in the list's order, of w lit (cos i if incidence else 1); the gradient is computed once and no sun scans the
    DSM.  tan_h, azimuths: horizon(dsm, grid, azimuths) of the same DSM; suns, weights, incidence as in sun_exposure.
    -> (gh, gw) float32, NaN at invalid cells; numpy if the DSM came as numpy, a device tensor otherwise."""
    azimuths = _azimuths_checked(azimuths)
    _interp_checked(interp)
    try:
        suns = [_sun_checked(*s) for s in suns]
    except TypeError:
        raise ValueError("suns must be a list of (azimuth, elevation) pairs, got %r" % (suns,)) from None
    if not suns:
        raise ValueError("sun_exposure_from_horizon needs at least one sun")
    weights = [1.0] * len(suns) if weights is None else [_finite(w, "a weight") for w in weights]
    if len(weights) != len(suns):
        raise ValueError("one weight per sun: %d suns, %d weights" % (len(suns), len(weights)))
    t, _ = _tan_h_checked(tan_h, azimuths)
    if tuple(t.shape[1:]) != (grid.height, grid.width):
        raise ValueError("tan_h shape %s differs from the grid's (%d, %d)" % (tuple(t.shape[1:]), grid.height, grid.width))
    z, as_numpy = _relief_input(dsm, grid)
    t = t.to(z.device)
    total = torch.zeros(z.shape, dtype=torch.float64, device=z.device)
    if incidence:
        dzde, dzdn = (g.double() for g in _gradient(z, grid, nodata))
    for (az, el), w in zip(suns, weights):
        hidden = _horizon_tangent(t, azimuths, az, interp) > math.tan(math.radians(el))      # horizon_lit == 2 (invalid cells: below)
        term = _cos_incidence(dzde, dzdn, az, el) * w if incidence else torch.full_like(total, w)
        total = total + torch.where(hidden, torch.zeros_like(term), term)
    ok = _valid_cells(z, nodata) & ~torch.isnan(t[0])
    return _back(as_numpy, torch.where(ok, total, torch.full_like(total, float("nan"))).float())


# ---- viewsheds: exact lines of sight from observers on or above the surface ------------------------------------------------------
MAX_VIEWSHED_OBSERVERS = 64                                       # observers of one smvs_dsm_viewshed call
VIEWSHED_MAX_SIDE = 65536                                         # cells along a side of the grid
VIEWSHED_MAX_UNITS = 1 << 23                                      # eye and target heights, in units of 2^-8 m (32768 m)
INVALID_OBSERVER = ("raise", "mark")


def viewshed_terms(grid, curvature=True, refraction=0.13, earth_radius=6371008.8, max_distance=None):
    """The four doubles smvs_dsm_viewshed and smvs_dsm_los take over `grid`: xres, yres, c256 = 256 (1 - refraction) / (2
    earth_radius) -- the drop of the surface below the observer's horizontal plane per squared metre of distance, in units
    of 2^-8 m, lessened by the bending of the ray; 0 without `curvature` -- and r2max = max_distance^2 [m^2], +inf for None.
    Checked against the limits of the entries.  -> (xres, yres, c256, r2max)."""
    _grid_checked(grid, "grid")
    gw, gh = int(grid.width), int(grid.height)
    if gw > VIEWSHED_MAX_SIDE or gh > VIEWSHED_MAX_SIDE:
        raise ValueError("a viewshed's grid has at most %d cells along a side, got %d x %d" % (VIEWSHED_MAX_SIDE, gw, gh))
    xres, yres = float(grid.xres), float(grid.yres)
    refraction = _finite(refraction, "refraction")
    if refraction > 1.0:
        raise ValueError("refraction must be at most 1, got %r" % refraction)
    earth_radius = _finite(earth_radius, "earth_radius")
    if not earth_radius > 0.0:
        raise ValueError("earth_radius must be > 0 [m], got %r" % earth_radius)
    c256 = 256.0 * (1.0 - refraction) / (2.0 * earth_radius) if curvature else 0.0
    w, h = gw * xres, gh * yres
    if not c256 * (w * w + h * h) < 2.0 ** 30:
        raise ValueError("the grid is too long for a viewshed: the drop across it must stay below 2^22 m")
    r2max = math.inf
    if max_distance is not None:
        max_distance = _finite(max_distance, "max_distance")
        r2max = max_distance * max_distance
        if not (max_distance > 0.0 and r2max > 0.0):
            raise ValueError("max_distance must be > 0 [m] or None, got %r" % max_distance)
    return xres, yres, c256, r2max


def _cells_checked(cells, shape, name):
    """An (m, 2) list of (row, col) with m >= 1, every cell on the grid -> int64 host array."""
    gh, gw = shape
    p = cells.cpu().numpy() if isinstance(cells, torch.Tensor) else np.asarray(cells)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError("%s is an (m, 2) list of (row, col) with m >= 1, got shape %s" % (name, tuple(p.shape)))
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError("%s (row, col) are integers, got %s" % (name, p.dtype))
    if int(p.min()) < 0 or int(p[:, 0].max()) >= gh or int(p[:, 1].max()) >= gw:
        raise ValueError("%s must lie on the %d x %d grid" % (name, gh, gw))
    return p.astype(np.int64)


def _height_units(h, m, name, lowest):
    """Heights [m], a number or one per item, as int32 units of 2^-8 m: rint(256 h), within lowest .. 2^23."""
    a = np.asarray(h, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(m, float(a))
    if a.shape != (m,):
        raise ValueError("%s is a number or one number per item (%d), got shape %s" % (name, m, tuple(a.shape)))
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite, got %r" % (name, h))
    units = np.rint(256.0 * a)
    if (units < lowest).any() or (units > VIEWSHED_MAX_UNITS).any():
        raise ValueError("%s must lie in %g .. 32768 m, got %r" % (name, lowest / 256.0, h))
    return units.astype(np.int32)


def _invalid_observers(z, rc, nodata):
    """Indices of the cells of rc (row, col) that hold no height by the rule of smvs_dsm_viewshed (one read of the device)."""
    at = torch.as_tensor(rc, device=z.device)
    zo = z[at[:, 0], at[:, 1]]
    ok = torch.isfinite(zo) & (zo != float(np.float32(nodata))) & (zo.abs() <= 32768.0)
    return (~ok).nonzero().flatten().cpu().tolist()


def viewshed(dsm, grid, observers, observer_height=1.6, target_height=0.0, absolute=False, max_distance=None, curvature=True,
             refraction=0.13, nodata=-999.0, return_above=False, invalid_observer="raise"):
    """Viewsheds of a DSM (include/satmvs.h smvs_dsm_viewshed, DESIGN.md section 9, "Viewshed"): for every observer of the
    list and every cell, whether an eye observer_height [m] above the observer's own cell (with `absolute`, at that height
    itself) sees a point target_height [m] above the cell, along one exact line of sight per cell: the cells the line steps
    through, heights in units of 2^-8 m, the earth's curvature and the `refraction` of the ray as a drop that grows with the
    squared distance (curvature=False: a flat earth), every comparison exact, grazing counted as seen.  observers: an (m, 2)
    list of (row, col) cells on the grid, m >= 1 (DSMGrid.cell_of gives them from map coordinates); the heights are numbers
    or one per observer, not negative unless absolute; max_distance [m] puts cells further away out of range.  More than 64
    observers go in chunks of 64; the bits do not depend on the chunking.  An observer that stands (not absolute) on a cell
    without a height raises ValueError; with invalid_observer="mark" its map is 0 everywhere instead, which tells it from any
    other observer's: an observer that stands sees at least its own cell (the entry's status words are not returned).  dsm (grid.height,
    grid.width) of any real dtype (taken as float32), numpy or a device tensor.
    -> seen (m, gh, gw) uint8: 0 no height, 1 seen, 2 hidden, 3 out of range (and, with return_above, above (m, gh, gw)
    float32: what must stand on a hidden cell [m] to be seen, 0 at seen cells, nodata at codes 0 and 3); numpy if the DSM came
    as numpy, device tensors otherwise."""
    xres, yres, c256, r2max = viewshed_terms(grid, curvature, refraction, max_distance=max_distance)
    if invalid_observer not in INVALID_OBSERVER:
        raise ValueError("invalid_observer must be one of %s, got %r" % (INVALID_OBSERVER, invalid_observer))
    rc = _cells_checked(observers, (grid.height, grid.width), "observers")
    m = rc.shape[0]
    eye = _height_units(observer_height, m, "observer_height", -VIEWSHED_MAX_UNITS if absolute else 0)
    tgt = _height_units(target_height, m, "target_height", 0)
    dsm = _dsm_converted(dsm, grid)
    z, as_numpy = _to_device(dsm, torch.float32)
    gh, gw = z.shape
    if not absolute and invalid_observer == "raise":
        bad = _invalid_observers(z, rc, nodata)
        if bad:
            raise ValueError("observer %d stands on cell (row %d, col %d), which holds no height" % (bad[0], rc[bad[0], 0], rc[bad[0], 1]))
    obs = np.stack([rc[:, 1], rc[:, 0], eye, np.full(m, 1 if absolute else 0), tgt], axis=1).astype(np.int32)
    nbytes = _lib.load().smvs_dsm_viewshed_workspace_bytes(gw, gh, min(m, MAX_VIEWSHED_OBSERVERS))
    if nbytes == 0:
        raise ValueError("unsupported viewshed: %d x %d cells" % (gw, gh))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
    seen = torch.empty((m, gh, gw), dtype=torch.uint8, device=z.device)
    above = torch.empty((m, gh, gw), dtype=torch.float32, device=z.device) if return_above else None
    status = torch.empty(m, dtype=torch.int32, device=z.device)
    for k0 in range(0, m, MAX_VIEWSHED_OBSERVERS):
        n = min(MAX_VIEWSHED_OBSERVERS, m - k0)
        _call(z.device, "smvs_dsm_viewshed", z, gw, gh, float(nodata), xres, yres, c256, r2max, np.ascontiguousarray(obs[k0:k0 + n]), n,
              seen[k0:k0 + n], None if above is None else above[k0:k0 + n], status[k0:k0 + n], ws, nbytes)
    seen, above = _back(as_numpy, seen, above)
    return (seen, above) if return_above else seen


def visibility_count(seen):
    """The cumulative viewshed: how many observers of viewshed()'s seen (m, gh, gw) uint8 see each cell (code 1), summed by
    torch on the device.  -> (gh, gw) int32, numpy or tensor as seen came."""
    as_numpy = not isinstance(seen, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(seen)) if as_numpy else seen
    if t.ndim != 3 or t.shape[0] < 1 or t.dtype != torch.uint8:
        raise ValueError("seen is (m, gh, gw) uint8 with m >= 1, got %s of shape %s" % (t.dtype, tuple(t.shape)))
    t, _ = _to_device(t)
    return _back(as_numpy, (t == 1).sum(dim=0, dtype=torch.int32))


def _los(z, grid, pairs, terms, nodata, return_above):
    """smvs_dsm_los over an (n, 7) int32 host array of pairs -> (seen (n) uint8, above (n) float32 or None) on z's device."""
    gh, gw = z.shape
    n = pairs.shape[0]
    if n >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 lines of sight go in one call, got %d" % n)
    p = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(z.device)
    seen = torch.empty(n, dtype=torch.uint8, device=z.device)
    above = torch.empty(n, dtype=torch.float32, device=z.device) if return_above else None
    _call(z.device, "smvs_dsm_los", z, gw, gh, float(nodata), terms[0], terms[1], terms[2], terms[3], p, n, seen, above)
    return seen, above


def line_of_sight(dsm, grid, a, b, observer_height=1.6, target_height=0.0, absolute=False, max_distance=None, curvature=True,
                  refraction=0.13, nodata=-999.0, return_above=False):
    """Lines of sight between pairs of cells by the rule of viewshed() (include/satmvs.h smvs_dsm_los): pair k has its eye
    observer_height above cell a[k] (with `absolute`, at that height) and its target target_height above cell b[k].  a, b:
    (m, 2) lists of (row, col) of equal length; the heights are numbers or one per pair.
    -> code (m) uint8: 0 no height at the target or (not absolute) under the observer, 1 seen, 2 hidden, 3 out of range (and,
    with return_above, above (m) float32 as in viewshed); numpy if the DSM came as numpy, device tensors otherwise."""
    terms = viewshed_terms(grid, curvature, refraction, max_distance=max_distance)
    shape = (grid.height, grid.width)
    a, b = _cells_checked(a, shape, "a"), _cells_checked(b, shape, "b")
    m = a.shape[0]
    if b.shape[0] != m:
        raise ValueError("a and b hold one cell per line of sight: %d and %d cells" % (m, b.shape[0]))
    eye = _height_units(observer_height, m, "observer_height", -VIEWSHED_MAX_UNITS if absolute else 0)
    tgt = _height_units(target_height, m, "target_height", 0)
    z, as_numpy = _to_device(_dsm_converted(dsm, grid), torch.float32)
    pairs = np.stack([a[:, 1], a[:, 0], eye, np.full(m, 1 if absolute else 0), b[:, 1], b[:, 0], tgt], axis=1)
    seen, above = _back(as_numpy, *_los(z, grid, pairs, terms, nodata, return_above))
    return (seen, above) if return_above else seen


def intervisibility(dsm, grid, points, height=1.6, max_distance=None, curvature=True, refraction=0.13, nodata=-999.0):
    """Which of `points` see each other: entry (i, j) is line_of_sight from `height` [m, a number >= 0] above points[i] to
    `height` above points[j], all m^2 lines in one smvs_dsm_los call.  The diagonal is 1 at points with a height; the matrix
    need not be symmetric (a line samples other cells than its reverse).  points: an (m, 2) list of (row, col).
    -> (m, m) uint8 with the codes of line_of_sight; numpy if the DSM came as numpy, a device tensor otherwise."""
    terms = viewshed_terms(grid, curvature, refraction, max_distance=max_distance)
    p = _cells_checked(points, (grid.height, grid.width), "points")
    m = p.shape[0]
    units = _height_units(height, 1, "height", 0)[0]
    z, as_numpy = _to_device(_dsm_converted(dsm, grid), torch.float32)
    i, j = np.repeat(np.arange(m), m), np.tile(np.arange(m), m)
    pairs = np.stack([p[i, 1], p[i, 0], np.full(m * m, units), np.zeros(m * m, np.int64), p[j, 1], p[j, 0], np.full(m * m, units)], axis=1)
    seen, _ = _los(z, grid, pairs, terms, nodata, False)
    return _back(as_numpy, seen.reshape(m, m))

"""Transverse Mercator projection (USGS series, Snyder), float64, on the native kernel (smvs_tm_project).

Same classes, constructor arguments and methods as the reference's tools/Transverse_Mercator.py: `Ellipsoid`,
`TransverseMercator(ellipsoid, latitude_origin, longitude_origin, scale_factor, False_Easting, False_Northing)` with
`proj(pts, reverse=False)`, `latlon2EastNorth(pts)` and `EastNorth2latlon(pts)`; points are (..., 2) = (lat, lon) in degrees or
(E, N) in metres.  numpy in gives numpy out; torch tensors on the GPU stay there.  There is no CPU fallback.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib


class Ellipsoid:
    """Reference ellipsoid; WGS84 by default."""

    def __init__(self, ellipsoid_a=6378137.000, inverse_flattening=298.257223563):
        self.a = float(ellipsoid_a)
        self.inv_f = float(inverse_flattening)
        self.f = 1.0 / self.inv_f
        self.b = self.a * (1 - self.f)
        self.e = math.sqrt(2 * self.f - self.f * self.f)
        self.sec_e = math.sqrt((self.e * self.e) / (1 - self.e * self.e))


class TransverseMercator:
    def __init__(self, ellipsoid, latitude_origin=0.0, longitude_origin=0.0,
                 scale_factor=1.0, False_Easting=500000.0, False_Northing=0.0):
        self.ellipsoid = ellipsoid
        self.a, self.b, self.f, self.e, self.sec_e = ellipsoid.a, ellipsoid.b, ellipsoid.f, ellipsoid.e, ellipsoid.sec_e
        self.lat0_org = float(latitude_origin)
        self.lon0_org = float(longitude_origin)
        self.k0 = float(scale_factor)
        self.FE = float(False_Easting)
        self.FN = float(False_Northing)

    def tm7(self):
        """The 7 parameters of the C ABI (include/satmvs.h): a, 1/f, lat0, lon0 [deg], k0, FE, FN."""
        return np.array([self.a, self.ellipsoid.inv_f, self.lat0_org, self.lon0_org, self.k0, self.FE, self.FN], dtype=np.float64)

    def proj(self, pts, reverse=False):
        """reverse False: (lat, lon) -> (E, N); True: (E, N) -> (lat, lon).  pts (..., 2); the result has the same shape."""
        return self._run(pts, 1 if reverse else 0)

    def latlon2EastNorth(self, pts):
        return self._run(pts, 0)

    def EastNorth2latlon(self, pts):
        return self._run(pts, 1)

    def _run(self, pts, direction):
        is_numpy = not isinstance(pts, torch.Tensor)
        t = torch.as_tensor(pts)
        if t.shape[-1] != 2:
            raise ValueError("points must have shape (..., 2), got %s" % (tuple(t.shape),))
        if is_numpy or not t.is_cuda:
            if not torch.cuda.is_available():
                raise _lib.SatMVSNativeError("TransverseMercator runs on an MI355X only (no CPU fallback)")
            dev = torch.device("cuda", torch.cuda.current_device())
        else:
            dev = t.device
        flat = t.to(device=dev, dtype=torch.float64).reshape(-1, 2)
        a, b = flat[:, 0].contiguous(), flat[:, 1].contiguous()
        o0, o1 = torch.empty_like(a), torch.empty_like(a)
        _lib.launch(dev, "smvs_tm_project", self.tm7(), a, b, o0, o1, a.numel(), direction)
        out = torch.stack((o0, o1), dim=-1).reshape(t.shape)
        return out.cpu().numpy() if is_numpy else out


def whu_tlc_projection():
    """The (non-real, planet-shifted) UTM projection of the WHU-TLC ground truth DSMs (WHU_TLC/readme.md): WGS84 ellipsoid,
    latitude of origin 0, central meridian -135, scale factor 0.9996, false easting 500000, false northing 0."""
    return TransverseMercator(Ellipsoid(6378137.0, 298.257223563), 0.0, -135.0, 0.9996, 500000.0, 0.0)

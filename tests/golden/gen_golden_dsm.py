"""Generate tests/golden/tm.npz by IMPORTING the reference's Transverse Mercator (tools/Transverse_Mercator.py).

Runs only where the reference checkout is (SATMVS_REFERENCE, read-only); the fixture is data: seeded points and the
reference's outputs.  Two projections: the WHU-TLC one (WHU_TLC/readme.md: WGS84, lat0 0, lon0 -135, k0 0.9996, FE 500000,
FN 0) and the reference's own example (lat0 0, lon0 123, k0 1, FE 500000).  Latitudes -60..60 deg, longitudes out to +-6 deg
from the central meridian; both directions (the inverse on the forward's output).

    python tests/golden/gen_golden_dsm.py
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SATMVS_REFERENCE", "/root/reference")


def main():
    spec = importlib.util.spec_from_file_location("ref_tm", os.path.join(REF, "tools", "Transverse_Mercator.py"))
    tm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tm)
    rng = np.random.default_rng(20261016)
    out = {}
    for name, (lat0, lon0, k0, fe, fn) in {"whu": (0.0, -135.0, 0.9996, 500000.0, 0.0),
                                           "example": (0.0, 123.0, 1.0, 500000.0, 0.0)}.items():
        proj = tm.TransverseMercator(tm.Ellipsoid(6378137.0, 298.257223563), lat0, lon0, k0, fe, fn)
        lat = np.concatenate([np.linspace(-60.0, 60.0, 121), rng.uniform(-60.0, 60.0, 1879)])
        lon = lon0 + np.concatenate([np.linspace(-6.0, 6.0, 121), rng.uniform(-6.0, 6.0, 1879)])
        ll = np.stack([lat, lon], -1)
        en = proj.proj(ll.copy(), False)
        back = proj.proj(en.copy(), True)
        out[name + ".tm7"] = np.array([6378137.0, 298.257223563, lat0, lon0, k0, fe, fn])
        out[name + ".latlon"] = ll
        out[name + ".en"] = en
        out[name + ".latlon_back"] = back
    np.savez_compressed(os.path.join(HERE, "tm.npz"), **out)
    print("wrote", os.path.join(HERE, "tm.npz"), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

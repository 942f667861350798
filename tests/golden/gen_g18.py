"""Generator of tests/golden/g18_tm_points.npz: transverse Mercator points on WGS84 / UTM evaluated with mpmath at 50 digits - the
geometry reference of the reprojection family (include/hsr_reproject.h).  Run it by hand (`python tests/golden/gen_g18.py`) or
import it: tests/test_reproject_host.py regenerates the fixture when mpmath is importable and compares; GPU tests read the file
and never import this module.

The series are Krueger's to n^6 (Karney 2011) with the coefficients as exact rationals, the conformal latitude is inverted by
Newton steps to convergence (not the kernel's three), and everything is rounded to float64 once, at the end.  Two facts hold the
series themselves (checked by the host test, see meridian_arc and round_trip): on the central meridian the northing is k0 times
the quadrature of the meridian arc, and inverse(forward) is the identity.

Each point: (E, N, lon0, FN) -> (lat, lon) by the inverse of the float64 E, N; and the forward direction (lat, lon) -> (fwd_E,
fwd_N) from the float64 lat, lon.  About 400 points: zones north and south, E in [1e5, 9e5], N up to 9.3e6, |lon - lon0| to 4
degrees, points on the central meridian and on the equator."""
import os

import numpy as np

DIGITS = 50
A_WGS84, INV_F, K0, FE = 6378137, "298.257223563", "0.9996", 500000
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g18_tm_points.npz")

# numerator / denominator per power n^1 .. n^6 (0 where the power is absent)
ALPHA = (((1, 2), (-2, 3), (5, 16), (41, 180), (-127, 288), (7891, 37800)),
         ((0, 1), (13, 48), (-3, 5), (557, 1440), (281, 630), (-1983433, 1935360)),
         ((0, 1), (0, 1), (61, 240), (-103, 140), (15061, 26880), (167603, 181440)),
         ((0, 1), (0, 1), (0, 1), (49561, 161280), (-179, 168), (6601661, 7257600)),
         ((0, 1), (0, 1), (0, 1), (0, 1), (34729, 80640), (-3418889, 1995840)),
         ((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (212378941, 319334400)))
BETA = (((1, 2), (-2, 3), (37, 96), (-1, 360), (-81, 512), (96199, 604800)),
        ((0, 1), (1, 48), (1, 15), (-437, 1440), (46, 105), (-1118711, 3870720)),
        ((0, 1), (0, 1), (17, 480), (-37, 840), (-209, 4480), (5569, 90720)),
        ((0, 1), (0, 1), (0, 1), (4397, 161280), (-11, 504), (-830251, 7257600)),
        ((0, 1), (0, 1), (0, 1), (0, 1), (4583, 161280), (-108847, 3991680)),
        ((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (20648693, 638668800)))


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


def constants():
    """(mp, n, k0 * A, e, alpha[6], beta[6]) at DIGITS digits."""
    mp = _mp()
    f = 1 / mp.mpf(INV_F)
    n = f / (2 - f)
    A = mp.mpf(A_WGS84) / (1 + n) * (1 + n ** 2 / 4 + n ** 4 / 64 + n ** 6 / 256)
    coef = lambda rows: [sum(mp.mpf(p) / q * n ** (k + 1) for k, (p, q) in enumerate(row)) for row in rows]  # noqa: E731
    return mp, n, mp.mpf(K0) * A, mp.sqrt(f * (2 - f)), coef(ALPHA), coef(BETA)


def _taup(mp, tau, e):
    sigma = mp.sinh(e * mp.atanh(e * tau / mp.sqrt(1 + tau * tau)))
    return tau * mp.sqrt(1 + sigma * sigma) - sigma * mp.sqrt(1 + tau * tau)


def forward(lat_deg, lon_deg, lon0, fn):
    """(E, N) as mpf."""
    mp, _, k0A, e, alpha, _ = constants()
    lam = mp.radians(mp.mpf(lon_deg) - mp.mpf(lon0))
    taup = _taup(mp, mp.tan(mp.radians(mp.mpf(lat_deg))), e)
    xip = mp.atan2(taup, mp.cos(lam))
    etap = mp.asinh(mp.sin(lam) / mp.sqrt(taup * taup + mp.cos(lam) ** 2))
    xi = xip + sum(a * mp.sin(2 * j * xip) * mp.cosh(2 * j * etap) for j, a in enumerate(alpha, start=1))
    eta = etap + sum(a * mp.cos(2 * j * xip) * mp.sinh(2 * j * etap) for j, a in enumerate(alpha, start=1))
    return FE + k0A * eta, mp.mpf(fn) + k0A * xi


def inverse(E, N, lon0, fn):
    """(lat_deg, lon_deg) as mpf."""
    mp, _, k0A, e, _, beta = constants()
    xi, eta = (mp.mpf(N) - mp.mpf(fn)) / k0A, (mp.mpf(E) - FE) / k0A
    xip = xi - sum(b * mp.sin(2 * j * xi) * mp.cosh(2 * j * eta) for j, b in enumerate(beta, start=1))
    etap = eta - sum(b * mp.cos(2 * j * xi) * mp.sinh(2 * j * eta) for j, b in enumerate(beta, start=1))
    taup = mp.sin(xip) / mp.sqrt(mp.sinh(etap) ** 2 + mp.cos(xip) ** 2)
    lam = mp.atan2(mp.sinh(etap), mp.cos(xip))
    e2m = 1 - e * e
    tau = taup
    for _ in range(12):
        ti = _taup(mp, tau, e)
        tau = tau + (taup - ti) / mp.sqrt(1 + ti * ti) * (1 + e2m * tau * tau) / (e2m * mp.sqrt(1 + tau * tau))
    return mp.degrees(mp.atan(tau)), mp.mpf(lon0) + mp.degrees(lam)


def meridian_arc(lat_deg):
    """The length of the meridian from the equator to lat_deg by quadrature of a (1 - e^2) / (1 - e^2 sin^2)^(3/2), as mpf."""
    mp, _, _, e, _, _ = constants()
    e2 = e * e
    return mp.quad(lambda p: A_WGS84 * (1 - e2) / (1 - e2 * mp.sin(p) ** 2) ** mp.mpf("1.5"), [0, mp.radians(mp.mpf(lat_deg))])


def sample_points():
    """The float64 inputs: (E, N, lon0, FN) rows, from a seeded generator and rounded to millimetres."""
    rng = np.random.default_rng(18)
    zones = [(-177.0, 0.0), (-117.0, 0.0), (3.0, 0.0), (45.0, 0.0), (177.0, 0.0), (-69.0, 1e7), (21.0, 1e7), (135.0, 1e7)]
    rows = []
    for k in range(200):                                                   # by latitude and longitude offset, |lambda| <= 4
        lon0, fn = zones[k % len(zones)]
        lat = rng.uniform(0.0, 84.0) if fn == 0.0 else -rng.uniform(0.0, 80.0)
        lam = rng.uniform(-4.0, 4.0) if k % 10 else (4.0 if k % 20 else -4.0)
        E, N = forward(lat, lon0 + lam, lon0, fn)
        rows.append((float(E), float(N), lon0, fn))
    for k in range(140):                                                   # by easting and northing
        lon0, fn = zones[(3 * k) % len(zones)]
        E = rng.uniform(1e5, 9e5) if k % 7 else (1e5 if k % 14 else 9e5)
        N = rng.uniform(0.0, 6.0e6) if fn == 0.0 else 1e7 - rng.uniform(0.0, 6.0e6)
        rows.append((E, N, lon0, fn))
    for k in range(30):                                                    # the central meridian, up to N = 9.3e6
        lon0, fn = zones[k % len(zones)]
        rows.append((5e5, 9.3e6 * (k + 1) / 30 if fn == 0.0 else 1e7 - 8.8e6 * (k + 1) / 30, lon0, fn))
    for k in range(30):                                                    # the equator
        lon0, fn = zones[k % len(zones)]
        rows.append((1e5 + 8e5 * k / 29, fn, lon0, fn))
    pts = np.array(rows, dtype=np.float64)
    pts[:, :2] = np.round(pts[:, :2], 3)
    return pts


def generate():
    pts = sample_points()
    lat, lon, fe, fnn = (np.empty(len(pts)) for _ in range(4))
    for i, (E, N, lon0, fn) in enumerate(pts):
        la, lo = inverse(E, N, lon0, fn)
        lat[i], lon[i] = float(la), float(lo)
        x, y = forward(lat[i], lon[i], lon0, fn)
        fe[i], fnn[i] = float(x), float(y)
    return dict(E=pts[:, 0].copy(), N=pts[:, 1].copy(), lon0=pts[:, 2].copy(), FN=pts[:, 3].copy(), lat=lat, lon=lon, fwd_E=fe,
                fwd_N=fnn)


if __name__ == "__main__":
    np.savez(PATH, **generate())
    print(f"wrote {PATH}")

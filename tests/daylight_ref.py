"""Float64 restatements for the daylight tests (TEST INFRASTRUCTURE): the camera
models (camera/{perspective,orthogonal,fishlens}.art), the CIE sky function
(light/cie.art), its host constants (CIELight.cpp:65-92) and the sun position
(skysun/SunLocation.cpp), written from the reference sources and independent
of the code under test.  Where the reference itself computes in float32 or
prints a number at six significant digits, so does this."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAYLIGHT = os.path.join(ROOT, "tests", "golden", "daylight")
KINDS = ["uniform", "cloudy", "clear", "intermediate"]
F32 = np.float32
FLT_EPS = float(np.finfo(np.float32).eps)
PI_F = float(F32(3.14159265359))  # flt_pi (core/common.art:7)


def printed(v):
    """A number as the generated shader text carries it (stream precision 6)."""
    return float("%g" % float(v))


# ---- sun position (SunLocation.cpp:17-104) ----------------------------------
def sun_ea(year=2020, month=5, day=6, hour=12, minute=0, seconds=0.0, latitude=49.235422, longitude=-6.9965744,
           timezone=-2.0):
    """(elevation, azimuth west of south) in radians; the reference's float
    constants Pi / Deg2Rad and its float cast of the sidereal angle are kept."""
    Pi = float(F32(3.14159265358979323846))
    Deg2Rad = float(F32(Pi) / F32(180.0))
    latitude, longitude, timezone = float(F32(latitude)), float(F32(longitude)), float(F32(timezone))
    dec_hours = hour + timezone + (minute + float(F32(seconds)) / 60.0) / 60.0
    idiv = lambda a, b: int(a / b)  # C integer division truncates
    aux1 = idiv(month - 14, 12)
    aux2 = (idiv(1461 * (year + 4800 + aux1), 4) + idiv(367 * (month - 2 - 12 * aux1), 12)
            - idiv(3 * idiv(year + 4900 + aux1, 100), 4) + day - 32075)
    days = float(aux2) - 0.5 + dec_hours / 24.0 - 2451545.0
    omega = 2.1429 - 0.0010394594 * days
    mean_longitude = 4.8950630 + 0.017202791698 * days
    anomaly = 6.2400600 + 0.0172019699 * days
    ecl_long = (mean_longitude + 0.03341607 * math.sin(anomaly) + 0.00034894 * math.sin(2 * anomaly) - 0.0001134
                - 0.0000203 * math.sin(omega))
    ecl_obl = 0.4090928 - 6.2140e-9 * days + 0.0000396 * math.cos(omega)
    ra = math.atan2(math.cos(ecl_obl) * math.sin(ecl_long), math.cos(ecl_long))
    if ra < 0:
        ra += float(F32(2) * F32(Pi))
    decl = math.asin(math.sin(ecl_obl) * math.sin(ecl_long))
    gmst = 6.6974243242 + 0.0657098283 * days + dec_hours
    lmst = float(F32(Deg2Rad) * F32(gmst * 15 - longitude))
    lat = float(F32(Deg2Rad) * F32(latitude))
    hour_angle = lmst - ra
    zenith = math.acos(math.cos(lat) * math.cos(hour_angle) * math.cos(decl) + math.sin(decl) * math.sin(lat))
    azimuth = math.atan2(-math.sin(hour_angle), math.tan(decl) * math.cos(lat) - math.sin(lat) * math.cos(hour_angle))
    if azimuth < 0:
        azimuth += float(F32(2) * F32(Pi))
    zenith += (6371.01 / 149597890) * math.sin(zenith)
    elevation = float(F32(1.57079632679489661923) - F32(zenith))
    return elevation, float(np.fmod(F32(azimuth) + F32(Pi), F32(2) * F32(Pi)))


def ea_direction(elevation, azimuth):
    """ElevationAzimuth::toDirectionYUp"""
    return np.array([math.cos(elevation) * math.sin(azimuth), math.sin(elevation), -math.cos(elevation) * math.cos(azimuth)])


# ---- CIE sky (CIELight.cpp, cie.art) -----------------------------------------
def sunny_constants(clear, elevation, sun_y, turbidity=2.45):
    """(zenith brightness / factor, c2) of CIELight.cpp:65-92, unprinted."""
    elevation = min(elevation, math.radians(87))
    zb = (1.376 * turbidity - 1.81) * math.tan(elevation) + 0.38
    if not clear:
        zb = (zb + 8.6 * sun_y + 0.123) / 2
    zb = max(0.0, zb * 1000 / 203)
    if clear:
        factor = 0.274 * (0.91 + 10 * math.exp(-3 * (math.pi / 2 - elevation)) + 0.45 * sun_y * sun_y)
        arr = [2.766521, 0.547665, -0.369832, 0.009237, 0.059229]
    else:
        factor = (2.739 + 0.9891 * math.sin(0.3119 + 2.6 * elevation)) * math.exp(-(math.pi / 2 - elevation) * (0.4441 + 1.48 * elevation))
        arr = [3.5556, -2.7152, -1.3081, 1.0660, 0.60227]
    x = (elevation - math.pi / 4) / (math.pi / 4)
    f = arr[4]
    for i in (3, 2, 1, 0):
        f = f * x + arr[i]
    norm_factor = f / math.pi / factor
    solar = 1.5e9 / 208 * (1.147 - 0.147 / max(sun_y, 0.16))
    additive = 6e-5 / math.pi * solar * sun_y * (1 if clear else 0.15)
    return zb / factor, zb * norm_factor + additive


class Sky:
    """The constants of one CIE sky as the reference's shader sees them."""

    def __init__(self, kind, has_ground=True, zenith=(1, 1, 1), ground=(1, 1, 1), scale=(1, 1, 1), ground_brightness=0.2,
                 sun_dir=(0, 1, 0), zenith_ratio=0.0, c2=0.0, transform=None):
        self.kind, self.has_ground = kind, has_ground
        self.zenith, self.ground, self.scale = (np.asarray(v, dtype=np.float64) for v in (zenith, ground, scale))
        self.ground_brightness = float(F32(ground_brightness))
        self.sun_dir = np.asarray(sun_dir, dtype=np.float64)
        self.zenith_ratio, self.c2 = zenith_ratio, c2
        self.transform = np.eye(3) if transform is None else np.asarray(transform, dtype=np.float64)

    @staticmethod
    def for_sun(kind, elevation, azimuth, **kw):
        sun = ea_direction(elevation, azimuth)
        zr, c2 = sunny_constants(kind == "clear", elevation, sun[1], kw.pop("turbidity", 2.45)) if kind in ("clear", "intermediate") else (0.0, 0.0)
        return Sky(kind, sun_dir=[printed(v) for v in sun], zenith_ratio=printed(zr), c2=printed(c2), **kw)

    def radiance(self, dirs):
        """L(d) for local (Y-up) unit directions, shape (n, 3) -> (n, 3)."""
        d = np.asarray(dirs, dtype=np.float64)
        ct = d[:, 1]
        a = (ct + float(F32(1.01))) ** 10
        f1, f2 = a * a / (a * a + 1), 1 / (a * a + 1)
        if self.kind in ("uniform", "cloudy"):
            cloudy = self.kind == "cloudy"
            c1 = (1 + 2 * ct) / 3 if cloudy else np.ones_like(ct)
            k2 = self.ground_brightness * (float(F32(0.777777777)) if cloudy else 1.0)
            scale = np.ones(3)
        else:
            cg = d @ self.sun_dir
            gamma = np.arccos(np.clip(cg, -1, 1))
            if self.kind == "clear":
                c = lambda v: float(F32(v))
                horizon = np.where(ct >= c(0.01), 1 - np.exp(-c(0.32) / np.where(ct >= c(0.01), ct, 1.0)), 1.0)
                c1 = (c(0.91) + 10 * np.exp(-3 * gamma) + c(0.45) * cg * cg) * horizon
            else:
                c = lambda v: float(F32(v))
                theta = np.arccos(np.clip(ct, -1, 1))
                st = math.acos(min(1.0, max(-1.0, self.sun_dir[1])))
                c1 = ((c(1.35) * np.sin(c(5.631) - c(3.59) * theta) + c(3.12)) * math.sin(c(4.396) - c(2.6) * st) + c(6.37) - theta) / c(2.326) \
                    * np.exp(gamma * -c(0.563) * ((c(2.629) - theta) * (c(1.562) - st) + c(0.812)))
            c1 = self.zenith_ratio * c1
            k2 = self.ground_brightness * self.c2
            scale = self.scale
        out = scale[None, :] * (self.zenith[None, :] * (c1 * f1)[:, None] + self.ground[None, :] * (k2 * f2)[:, None])
        if not self.has_ground:
            out[ct < 0] = 0
        return out

    def world_radiance(self, dirs):
        """Light::emission for world directions leaving the scene (env.art:48-55, 88)."""
        local = np.asarray(dirs, dtype=np.float64) @ self.transform.T
        out = self.radiance(local)
        if not self.has_ground:
            out[local[:, 1] <= FLT_EPS] = 0
        return out


# the fixture scenes' sun: 2022-11-18 13:00, Saarbruecken, timezone -1
FIXTURE_SUN = dict(year=2022, month=11, day=18, hour=13, minute=0, seconds=0, latitude=49.235422, longitude=-6.9965744,
                   timezone=-1)


def fixture_sky(kind):
    if kind in ("uniform", "cloudy"):
        return Sky(kind)
    return Sky.for_sun(kind, *sun_ea(**FIXTURE_SUN))


# ---- cameras -------------------------------------------------------------------
class Camera:
    """eye / dir / up as the loader's desc gives them; rays for normalised
    pixel coordinates nx, ny in [-1, 1] (ny up) on a width x height film."""

    def __init__(self, kind, eye, dir, up, width, height, fov=math.radians(60), vertical_fov=False, aspect=None, scale=1.0,
                 aperture=0.0, focal=1.0):
        self.kind = kind
        self.eye, self.dir, self.up = (np.asarray(v, dtype=np.float64) for v in (eye, dir, up))
        r = np.cross(self.dir, self.up)
        self.right = r / np.linalg.norm(r)
        asp = width / height
        a = asp if aspect is None else aspect
        if kind == "orthogonal":
            self.sx, self.sy = scale, scale / a
        elif vertical_fov:
            self.sy = math.tan(fov / 2)
            self.sx = self.sy * a
        else:
            self.sx = math.tan(fov / 2)
            self.sy = self.sx / a
        self.xasp = 1.0 if asp < 1 else asp
        self.yasp = 1.0 if asp > 1 else asp
        self.aperture, self.focal = aperture, focal

    def to_world(self, x, y, z):
        return x[:, None] * self.right[None] + y[:, None] * self.up[None] + z[:, None] * self.dir[None]

    def rays(self, nx, ny, lens_u=None, lens_v=None):
        nx, ny = np.asarray(nx, dtype=np.float64).ravel(), np.asarray(ny, dtype=np.float64).ravel()
        n = nx.size
        unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
        if self.kind == "orthogonal":
            return self.eye[None] + self.to_world(self.sx * nx, self.sy * ny, np.zeros(n)), np.tile(self.dir, (n, 1))
        if self.kind == "fishlens":
            fx, fy = nx * self.xasp, ny * self.yasp
            r = np.sqrt(fx * fx + fy * fy)
            theta = r * PI_F / 2
            safe = np.where(r < FLT_EPS, 1.0, r)
            sp, cp = np.where(r < FLT_EPS, 0.0, fy / safe), np.where(r < FLT_EPS, 0.0, fx / safe)
            return np.tile(self.eye, (n, 1)), unit(self.to_world(np.sin(theta) * cp, np.sin(theta) * sp, np.cos(theta)))
        d = unit(self.to_world(self.sx * nx, self.sy * ny, np.ones(n)))
        if self.aperture <= FLT_EPS:
            return np.tile(self.eye, (n, 1)), d
        ax, ay = concentric_disk(lens_u, lens_v)
        ap = self.to_world(ax * self.aperture, ay * self.aperture, np.zeros(n))
        return self.eye[None] + ap, unit(d * self.focal - ap)


def concentric_disk(u, v):
    """square_to_concentric_disk (core/warp.art:2-22)"""
    a, b = 2 * np.asarray(u, dtype=np.float64) - 1, 2 * np.asarray(v, dtype=np.float64) - 1
    first = a * a > b * b
    sdiv = lambda p, q: np.where(np.abs(q) <= FLT_EPS, 0.0, p / np.where(np.abs(q) <= FLT_EPS, 1.0, q))
    phi = np.where(first, (PI_F / 4) * sdiv(b, a), PI_F / 2 - (PI_F / 4) * sdiv(a, b))
    rad = np.where(first, a, b)
    x, y = np.cos(phi) * rad, np.sin(phi) * rad
    zero = (a == 0) & (b == 0)
    return np.where(zero, 0.0, x), np.where(zero, 0.0, y)


def fishlens_sky_image(sky, size=256, sub=4):
    """The fixture view (eye 0, dir +Y, up +Z, so right = dir x up = +X) of a sky,
    sub x sub stratified samples per pixel: (size, size, 3) float64."""
    cam = Camera("fishlens", [0, 0, 0], [0, 1, 0], [0, 0, 1], size, size)
    img = np.zeros((size, size, 3))
    ys, xs = np.mgrid[0:size, 0:size]
    for sy in range(sub):
        for sx in range(sub):
            nx = 2 * (xs + (sx + 0.5) / sub) / size - 1
            ny = 1 - 2 * (ys + (sy + 0.5) / sub) / size
            _, d = cam.rays(nx, ny)
            img += sky.world_radiance(d).reshape(size, size, 3)
    return img / (sub * sub)

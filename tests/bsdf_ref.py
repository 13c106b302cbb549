"""The shading models in numpy float64, vectorised over rays, written from the
reference's artic text (bsdf/*.art, core/microfacet.art, core/fresnel.art,
core/shading.art, core/sampling.art, core/warp.art) and from nothing else: no
GPU, no project code.  Every function names the lines it restates.

A ray is a row.  Vectors are (n, 3) arrays, colours (n, 3), flags (n,) bool.
Both branches of every `if` are computed for all rays and chosen with
np.where; a Trace notes the rays for which some branch decision lies within
1e-5 of its threshold, so that a test can leave them out.

`mutant=` swaps in one deliberate porting slip (MUTANTS); the tests use them to
show that their tolerance cannot hide one.
"""
import math

import numpy as np

FLT_EPS = 1.1920928955e-07  # core/common.art:3
PI = math.pi
REL = 1e-5  # a branch decision closer than this to its threshold is not replayed

MUTANTS = ("g1_exchanged", "alpha_exchanged", "eta_not_inverted", "jacobian_eta_inverted", "plastic_mix_at_cos_in",
           "oren_nayar_c_kd", "sheen_base_color", "textbook_conductor", "vndf_pdf_without_g1")

# igx_material.bsdf_type, igx_material.distribution (include/igx_scene.h)
DIFFUSE, DIELECTRIC, CONDUCTOR, PLASTIC, PRINCIPLED = range(5)
MF_DELTA, MF_VNDF_GGX, MF_GGX, MF_BECKMANN = range(4)

np.seterr(all="ignore")  # unused branches divide by zero; np.where drops them


# ---- bookkeeping ---------------------------------------------------------------------------
class Trace:
    """Which rays had a branch decision too close to call.  Thresholds are
    compared on the scale max(|threshold|, 1): cosines, random numbers, Fresnel
    factors and lobe probabilities are all of unit scale."""

    def __init__(self, n):
        self.unstable = np.zeros(n, bool)
        self.ill = np.zeros(n, bool)  # see Microfacet.sample

    def _note(self, a, b, active):
        near = np.abs(a - b) <= REL * np.maximum(np.abs(b), 1.0)
        self.unstable |= near & active & np.isfinite(a)

    def lt(self, a, b, active=True):
        self._note(a, b, active)
        return a < b

    def le(self, a, b, active=True):
        self._note(a, b, active)
        return a <= b

    def gt(self, a, b, active=True):
        self._note(a, b, active)
        return a > b

    def ge(self, a, b, active=True):
        self._note(a, b, active)
        return a >= b


class Draws:
    """The random numbers of every ray's path, (n, k), with one cursor per ray:
    next(active) hands every ray its next number and moves the cursor of the
    active ones."""

    def __init__(self, table, start=0):
        self.table = np.asarray(table, np.float64)
        self.cur = np.full(self.table.shape[0], start, np.int64)

    def next(self, active=True):
        k = self.table.shape[1]
        assert (self.cur[np.broadcast_to(active, self.cur.shape)] < k).all(), "draw table too short"
        v = self.table[np.arange(len(self.cur)), np.minimum(self.cur, k - 1)]
        self.cur = self.cur + np.broadcast_to(active, self.cur.shape).astype(np.int64)
        return v


# ---- vectors (core/vector.art:122-144, core/common.art:147-171) ----------------------------
def vec(x, y, z):
    return np.stack(np.broadcast_arrays(x, y, z), axis=-1).astype(np.float64)


def dot(a, b):
    return (a * b).sum(axis=-1)


def normalize(v):
    return v * (1 / np.sqrt(dot(v, v)))[..., None]


def reflect(v, n):  # vector.art:126
    return n * (2 * dot(n, v))[..., None] - v


def refract(v, n, eta, cos_i, cos_t):  # vector.art:129
    return n * (eta * cos_i - cos_t)[..., None] - v * np.asarray(eta)[..., None]


def halfway(a, b):  # vector.art:143
    return normalize(a + b)


def halfway_refractive(a, b, eta):  # vector.art:144
    return normalize(a + b * np.asarray(eta, np.float64)[..., None])


def safe_div(a, b):  # common.art:169
    return np.where(np.abs(b) <= FLT_EPS, 0.0, a / b)


def safe_sqrt(a):  # common.art:171
    return np.sqrt(np.maximum(0.0, a))


def lerp(a, b, k):  # common.art:120-122, color.art:18-22
    return (1 - k) * a + k * b


def col(c, f):
    return np.asarray(c, np.float64) * np.asarray(f, np.float64)[..., None]


def luminance(c):  # color.art:28
    return c[..., 0] * 0.2126 + c[..., 1] * 0.7152 + c[..., 2] * 0.0722


# ---- the shading frame (core/matrix.art:20-28, core/shading.art:8-9) -----------------------
class Frame:
    def __init__(self, n):
        n = np.asarray(n, np.float64)
        sign = np.copysign(1.0, n[..., 2])
        a = -1 / (sign + n[..., 2])
        b = n[..., 0] * n[..., 1] * a
        self.t = vec(1 + sign * n[..., 0] * n[..., 0] * a, sign * b, -sign * n[..., 0])
        self.bt = vec(b, sign + n[..., 1] * n[..., 1] * a, -n[..., 1])
        self.n = n

    def to_local(self, v):
        return vec(dot(self.t, v), dot(self.bt, v), dot(self.n, v))

    def to_world(self, v):
        return self.t * v[..., 0:1] + self.bt * v[..., 1:2] + self.n * v[..., 2:3]


class Surface:
    """SurfaceElement of shapes/trimesh.art:26-37 for a flat face: the frame is
    built from the normal turned towards the ray's side."""

    def __init__(self, normal, ray_dir, point):
        normal = np.broadcast_to(np.asarray(normal, np.float64), ray_dir.shape)
        self.entering = dot(ray_dir, normal) <= 0
        self.local = Frame(np.where(self.entering[:, None], normal, -normal))
        self.point = point


# ---- samplers (core/sampling.art:12-20, 62-69; core/warp.art:2-22, 63-91) ------------------
def sample_cosine_hemisphere(u, v):
    c, s, phi = safe_sqrt(v), safe_sqrt(1 - v), 2 * PI * u
    return vec(s * np.cos(phi), s * np.sin(phi), c), c / PI


def square_to_concentric_disk(x, y):
    a, b = 2 * x - 1, 2 * y - 1
    top = a * a > b * b
    phi = np.where(top, (PI / 4) * safe_div(b, a), (PI / 2) - (PI / 4) * safe_div(a, b))
    r = np.where(top, a, b)
    zero = (a == 0) & (b == 0)
    return np.where(zero, 0.0, np.cos(phi) * r), np.where(zero, 0.0, np.sin(phi) * r)


def equal_area_square_to_sphere(x, y):
    u, v = 2 * x - 1, 2 * y - 1
    au, av = np.abs(u), np.abs(v)
    sd = 1 - (au + av)
    r = 1 - np.abs(sd)
    phi = np.where(r == 0, 1.0, (av - au) / r + 1) * PI / 4
    cos_theta = np.copysign(1 - r * r, sd)
    sin_theta = safe_sqrt(2 - r * r) * r
    return vec(np.copysign(np.cos(phi), u) * sin_theta, np.copysign(np.sin(phi), v) * sin_theta, cos_theta)


# ---- Fresnel (core/fresnel.art) -------------------------------------------------------------
def fresnel(eta, cos_i, tr=None, active=True):
    """fresnel(), fresnel.art:7-27: (is Some, cos_t, factor)."""
    eta = np.asarray(eta, np.float64)
    eta2 = np.where(cos_i < 0, 1 / eta, eta)
    cos2_t = 1 - (1 - cos_i * cos_i) * eta2 * eta2
    none = tr.le(cos2_t, 0.0, active) if tr is not None else cos2_t <= 0
    cos_t = np.sqrt(np.maximum(cos2_t, 0))
    ci = np.abs(cos_i)
    r_s = safe_div(eta2 * ci - cos_t, eta2 * ci + cos_t)
    r_p = safe_div(ci - eta2 * cos_t, ci + eta2 * cos_t)
    factor = np.clip((r_s * r_s + r_p * r_p) * 0.5, 0, 1)
    return ~none, np.where(cos_i < 0, -cos_t, cos_t), factor


def fresnel_dielectric(eta, cos_i):  # core/math.art:120-123
    some, _, f = fresnel(eta, cos_i)
    return np.where(some, f, 1.0)


def conductor_factor(n, k, cos_i, mutant=None):
    """fresnel.art:29-36, the reference's own form; the textbook one as a mutant."""
    if mutant == "textbook_conductor":
        c2 = cos_i * cos_i
        s2 = 1 - c2
        t0 = n * n - k * k - s2
        a2b2 = np.sqrt(t0 * t0 + 4 * n * n * k * k)
        t1 = a2b2 + c2
        t2 = 2 * np.sqrt(0.5 * (a2b2 + t0)) * cos_i
        rs = (t1 - t2) / (t1 + t2)
        t3, t4 = c2 * a2b2 + s2 * s2, t2 * s2
        return np.clip(0.5 * (rs * (t3 - t4) / (t3 + t4) + rs), 0, 1)
    f = n * n + k * k
    d1 = f * cos_i * cos_i
    d2 = 2.0 * n * cos_i
    r_s = safe_div(d1 - d2, d1 + d2)
    r_p = safe_div(f - d2 + cos_i * cos_i, f + d2 + cos_i * cos_i)
    return np.clip((r_s * r_s + r_p * r_p) * 0.5, 0, 1)


def fresnel_diffuse_factor(eta):  # fresnel.art:42-64
    if eta < 1:
        return -1.4399 * (eta * eta) + 0.7099 * eta + 0.6681 + 0.0636 / eta
    i1 = 1 / eta
    return 0.919317 - 3.4793 * i1 + 6.75335 * i1 ** 2 - 7.80989 * i1 ** 3 + 4.98554 * i1 ** 4 - 1.36881 * i1 ** 5


def schlick_approx(f):  # fresnel.art:88-91
    s = np.clip(1 - f, 0, 1)
    return (s * s) * (s * s) * s


def schlick_r0(eta):  # fresnel.art:101-104
    f = np.clip((eta - 1) / (eta + 1), -1, 1)
    return f * f


# ---- Jacobians of the half-direction mappings (core/shading.art:68-74) ----------------------
def reflective_jacobian(cos):
    return safe_div(1.0, 4 * cos)


def refractive_jacobian(eta, cos_i, cos_o, mutant=None):
    if mutant == "jacobian_eta_inverted":
        eta = 1 / eta
    d = cos_i + cos_o * eta
    return safe_div(eta * eta * cos_i, d * d)


# ---- microfacet models on vectors of the shading frame (core/microfacet.art) ---------------
def g_1_walter(w, au, av):  # microfacet.art:135-156
    k2 = ((au * w[..., 0]) ** 2 + (av * w[..., 1]) ** 2) / (w[..., 2] * w[..., 2])
    a, a2 = 1 / np.sqrt(k2), 1 / k2
    g = np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a2) / (1.0 + 2.276 * a + 2.577 * a2))
    return np.where(np.abs(w[..., 2]) <= FLT_EPS, 0.0, np.where(k2 <= FLT_EPS, 1.0, g))


def g_1_smith(w, au, av):  # microfacet.art:158-175
    a2 = (au * w[..., 0]) ** 2 + (av * w[..., 1]) ** 2
    g = 2 / (1 + np.sqrt(1 + a2 / (w[..., 2] * w[..., 2])))
    return np.where(np.abs(w[..., 2]) <= FLT_EPS, 0.0, np.where(a2 <= FLT_EPS, 1.0, g))


def ndf_beckmann(m, au, av):  # microfacet.art:177-187
    cz = m[..., 2]
    k2 = safe_div((m[..., 0] / au) ** 2 + (m[..., 1] / av) ** 2, cz * cz)
    return safe_div(np.exp(-k2), PI * au * av * cz * cz * cz * cz)


def ndf_ggx(m, au, av):  # microfacet.art:189-199
    k = (m[..., 0] / au) ** 2 + (m[..., 1] / av) ** 2 + m[..., 2] ** 2
    return safe_div(1.0, PI * au * av * k * k)


def sin_cos_phi(v):  # shading.art:41-48
    d = safe_sqrt(1 - v[..., 2] * v[..., 2])
    ok = np.abs(d) > FLT_EPS
    return np.where(ok, v[..., 1] / d, 0.0), np.where(ok, v[..., 0] / d, 1.0)


class Microfacet:
    """MicrofacetDistribution (microfacet.art:274-395) of kind MF_VNDF_GGX, MF_GGX or MF_BECKMANN."""

    def __init__(self, kind, au, av, mutant=None):
        if mutant == "alpha_exchanged":
            au, av = av, au
        self.kind, self.au, self.av, self.mutant = kind, float(au), float(av), mutant
        self.is_delta = kind == MF_DELTA or au <= 1e-4 or av <= 1e-4  # microfacet.art:298

    def D(self, m):
        return ndf_beckmann(m, self.au, self.av) if self.kind == MF_BECKMANN else ndf_ggx(m, self.au, self.av)

    def G1(self, w):
        walter = self.kind == MF_BECKMANN
        if self.mutant == "g1_exchanged":
            walter = not walter
        return g_1_walter(w, self.au, self.av) if walter else g_1_smith(w, self.au, self.av)

    def G(self, wi, wo, m):
        return self.G1(wi) * self.G1(wo)

    def pdf(self, wi, wo, m):
        if self.is_delta:  # make_delta_model, microfacet.art:201-210: D = 0
            return np.zeros(m.shape[:-1])
        if self.kind == MF_VNDF_GGX:  # pdf_vndf_ggx, microfacet.art:368-371
            g1 = 1.0 if self.mutant == "vndf_pdf_without_g1" else self.G1(wo)
            return safe_div(g1 * np.abs(dot(wo, m)) * self.D(m), np.abs(wo[..., 2]))
        return self.D(m) * np.abs(m[..., 2])  # microfacet.art:291

    def sample(self, rnd, wo, active, tr=None):
        """(normal in the shading frame, pdf); two numbers either way.

        The VNDF sampler takes sin and cos of the stretched view direction's
        azimuth from sqrt(1 - z^2) (sin_cos_phi, shading.art:41-48).  For a
        small roughness or a view along the normal z^2 is close to 1, and the
        float32 difference carries a relative error of 2^-24 / (1 - z^2) before
        anything else is rounded; the slopes, and with them D at the sampled
        normal, inherit it.  The reference has that error as well (it computes
        in float32); a float64 replay has not.  `tr.ill` marks the rays where it
        exceeds 1e-4: they are compared, with an allowance of their own."""
        u0, u1 = rnd.next(active), rnd.next(active)
        au, av = self.au, self.av
        if self.kind == MF_VNDF_GGX:  # sample_vndf_ggx(_11), microfacet.art:321-366
            sl = normalize(vec(au * wo[..., 0], av * wo[..., 1], wo[..., 2]))
            if tr is not None:
                tr.ill |= active & (1 - sl[..., 2] * sl[..., 2] < 1e4 * 2.0 ** -24)
            sin_phi, cos_phi = sin_cos_phi(sl)
            cos_theta = np.abs(sl[..., 2])
            px, py = square_to_concentric_disk(u0, u1)
            s = 0.5 * (1 + cos_theta)
            y = (1 - s) * safe_sqrt(1 - px * px) + s * py
            z = safe_sqrt(1 - y * y - px * px)
            sin_theta = safe_sqrt(1 - cos_theta * cos_theta)
            norm = safe_div(1.0, sin_theta * y + cos_theta * z)
            sx, sy = (cos_theta * y - sin_theta * z) * norm, px * norm
            s2x = (cos_phi * sx - sin_phi * sy) * au
            s2y = (sin_phi * sx + cos_phi * sy) * av
            m = np.where(np.isfinite(s2x)[:, None], normalize(vec(-s2x, -s2y, 1.0)), 0.0)
            return m, self.pdf(None, wo, m)
        ar = av / au
        if self.kind == MF_GGX and au == av:  # microfacet.art:249
            phi = 2 * PI * u1
        else:
            phi = np.arctan(ar * np.tan(2 * PI * u1))
        cos_phi = np.cos(phi)
        sin_phi = np.sqrt(1 - cos_phi * cos_phi)
        kx, ky = cos_phi / au, sin_phi / av
        d2 = kx * kx + ky * ky
        if self.kind == MF_BECKMANN:  # microfacet.art:215-235
            cos_theta = 1 / np.sqrt(1 - (1 / d2) * np.log(1.0 - u0))
            c2 = cos_theta * cos_theta
            pdf = (1 - u0) / (PI * au * av * c2 * cos_theta)
        else:  # microfacet.art:244-267
            t2 = safe_div(1.0, d2) * u0 / (1 - u0)
            cos_theta = 1 / np.sqrt(1 + t2)
            c2 = cos_theta * cos_theta
            k2 = d2 * (1 - c2) / c2  # sinTheta^2 = 1 - cosTheta2
            pdf = safe_div(1.0, PI * au * av * c2 * cos_theta * (1 + k2) * (1 + k2))
        sin_theta = np.sqrt(1 - c2)
        return vec(sin_theta * cos_phi, sin_theta * sin_phi, cos_theta), pdf


# ---- the BSDFs --------------------------------------------------------------------------------
class Sample:
    def __init__(self, n):
        self.dir = np.zeros((n, 3))
        self.color = np.zeros((n, 3))
        self.pdf = np.zeros(n)
        self.eta = np.ones(n)
        self.valid = np.zeros(n, bool)

    def put(self, mask, dir, color, pdf, eta=1.0):
        mask = np.broadcast_to(mask, self.valid.shape)
        self.dir = np.where(mask[:, None], dir, self.dir)
        self.color = np.where(mask[:, None], color, self.color)
        self.pdf = np.where(mask, pdf, self.pdf)
        self.eta = np.where(mask, eta, self.eta)
        self.valid = self.valid | mask
        return self

    def merge(self, mask, other):
        return self.put(mask & other.valid, other.dir, other.color, other.pdf, other.eta)


class Bsdf:
    """in and out are world vectors; eval includes |cos_in| (driver/bsdf.art:1-20)."""
    is_specular = False

    def __init__(self, surf, tr=None):
        self.surf, self.L = surf, surf.local
        self.n = len(surf.entering)
        self.tr = tr if tr is not None else Trace(self.n)

    def eval(self, wi, wo, active=True):
        return np.zeros((self.n, 3))

    def pdf(self, wi, wo, active=True):
        return np.zeros(self.n)


class Lambert(Bsdf):  # diffuse.art:2-11
    def __init__(self, surf, kd, tr=None):
        super().__init__(surf, tr)
        self.kd = np.asarray(kd, np.float64)

    def eval(self, wi, wo, active=True):
        return col(self.kd, np.abs(dot(wi, self.L.n)) / PI)

    def pdf(self, wi, wo, active=True):
        return np.maximum(dot(wi, self.L.n), 0) / PI

    def sample(self, rnd, wo, active):
        d, pdf = sample_cosine_hemisphere(rnd.next(active), rnd.next(active))
        return Sample(self.n).put(active, self.L.to_world(d), np.broadcast_to(self.kd, (self.n, 3)), pdf)


class OrenNayar(Lambert):  # diffuse.art:15-39
    def __init__(self, surf, alpha, kd, tr=None, mutant=None):
        super().__init__(surf, kd, tr)
        self.a2, self.mutant = alpha * alpha, mutant

    def eval(self, wi, wo, active=True):
        p1, p2 = np.abs(dot(wi, self.L.n)), np.abs(dot(wo, self.L.n))
        s = -p1 * p2 + np.maximum(dot(wo, wi), 0)
        t = np.where(s <= FLT_EPS, 1.0, np.maximum(FLT_EPS, np.maximum(p1, p2)))
        a2 = self.a2
        A, B, C = 1 - 0.5 * a2 / (a2 + 0.33), 0.45 * a2 / (a2 + 0.09), 0.17 * a2 / (a2 + 0.13)
        kd2 = self.kd if self.mutant == "oren_nayar_c_kd" else self.kd * self.kd
        return (col(self.kd, (A + B * s / t) / PI) + kd2 * (C / PI)) * p1[:, None]

    def sample(self, rnd, wo, active):
        d, pdf = sample_cosine_hemisphere(rnd.next(active), rnd.next(active))
        g = self.L.to_world(d)
        return Sample(self.n).put(active, g, self.eval(g, wo) * (1 / pdf)[:, None], pdf)


class Mirror(Bsdf):  # conductor.art:2-9
    is_specular = True

    def __init__(self, surf, ks, tr=None):
        super().__init__(surf, tr)
        self.ks = np.asarray(ks, np.float64)

    def sample(self, rnd, wo, active):
        return Sample(self.n).put(active, reflect(wo, self.L.n), np.broadcast_to(self.ks, (self.n, 3)), 1.0)


class PureConductor(Bsdf):  # conductor.art:13-30
    is_specular = True

    def __init__(self, surf, eta, k, ks, tr=None, mutant=None):
        super().__init__(surf, tr)
        self.eta, self.k, self.ks = (np.asarray(v, np.float64) for v in (eta, k, ks))
        self.mutant = mutant

    def sample(self, rnd, wo, active):
        c = dot(wo, self.L.n)
        f = np.stack([conductor_factor(self.eta[i], self.k[i], c, self.mutant) for i in range(3)], axis=-1)
        return Sample(self.n).put(active, reflect(wo, self.L.n), self.ks * f, 1.0)


class RoughConductor(Bsdf):  # conductor.art:34-109, kd black
    def __init__(self, surf, eta, k, ks, micro, tr=None, mutant=None):
        super().__init__(surf, tr)
        self.eta, self.k, self.ks = (np.asarray(v, np.float64) for v in (eta, k, ks))
        self.micro, self.mutant = micro, mutant

    def fresnel_term(self, c):
        return np.stack([conductor_factor(self.eta[i], self.k[i], c, self.mutant) for i in range(3)], axis=-1)

    def eval(self, wi, wo, active=True):
        li, lo = self.L.to_local(wi), self.L.to_local(wo)
        cos_o, cos_i = np.abs(lo[:, 2]), np.abs(li[:, 2])
        black = self.tr.le(cos_o, FLT_EPS, active) | self.tr.le(cos_i, FLT_EPS, active)
        h = halfway(li, lo)
        f = self.fresnel_term(np.abs(dot(lo, h)))
        v = col(self.ks * f, self.micro.D(h) * self.micro.G(li, lo, h) / (4 * cos_o))
        return np.where(black[:, None], 0.0, v)

    def pdf(self, wi, wo, active=True):
        li, lo = self.L.to_local(wi), self.L.to_local(wo)
        h = halfway(li, lo)
        return self.micro.pdf(li, lo, h) * safe_div(1.0, 4 * np.abs(dot(lo, h)))

    def sample(self, rnd, wo, active):
        lo = self.L.to_local(wo)
        ok = active & ~self.tr.le(np.abs(lo[:, 2]), FLT_EPS, active)
        m, mpdf = self.micro.sample(rnd, lo, ok, self.tr)
        ok = ok & ~(dot(m, m) <= FLT_EPS)
        oh = normalize(m)
        h = np.where(self.tr.lt(dot(oh, lo), 0.0, ok)[:, None], -oh, oh)
        li = reflect(lo, h)
        ok = ok & ~self.tr.le(np.abs(li[:, 2]), FLT_EPS, ok)
        pdf = mpdf * (1 / (4 * np.abs(dot(lo, h))))
        wi = self.L.to_world(li)
        return Sample(self.n).put(ok, wi, self.eval(wi, wo, ok) * safe_div(1.0, pdf)[:, None], pdf)


def make_conductor(surf, eta, k, ks, micro, tr, mutant):  # conductor.art:112-122
    if micro.is_delta:
        if np.all(np.abs(np.asarray(eta)) <= 1e-4) and np.all(np.abs(np.asarray(k) - 1) <= 1e-4):
            return Mirror(surf, ks, tr)
        return PureConductor(surf, eta, k, ks, tr, mutant)
    return RoughConductor(surf, eta, k, ks, micro, tr, mutant)


class VariadicMix(Bsdf):
    """make_variadic_mix_bsdf, mix.art:2-72, with mix_f(out_dir)."""

    def __init__(self, mat1, mat2, mix_f, tr, mix_eval=None):
        super().__init__(mat1.surf, tr)
        self.m1, self.m2, self.mix_f = mat1, mat2, mix_f
        self.mix_eval = mix_eval or (lambda wi, wo: mix_f(wo))  # the mutant's hook
        self.is_specular = mat1.is_specular and mat2.is_specular

    def _mix(self, a, b, k):
        kk = k[:, None] if a.ndim == 2 else k
        return np.where(kk <= 0, a, np.where(kk >= 1, b, lerp(a, b, kk)))

    def eval(self, wi, wo, active=True):
        return self._mix(self.m1.eval(wi, wo, active), self.m2.eval(wi, wo, active), self.mix_eval(wi, wo))

    def pdf(self, wi, wo, active=True):
        return self._mix(self.m1.pdf(wi, wo, active), self.m2.pdf(wi, wo, active), self.mix_eval(wi, wo))

    def _sample_mat(self, rnd, wo, active, first, second, t):  # mix.art:33-47
        s = first.sample(rnd, wo, active)
        if second.is_specular:
            return s
        ok = active & s.valid
        p = lerp(s.pdf, second.pdf(s.dir, wo, ok), t)
        c = lerp(s.color * s.pdf[:, None], second.eval(s.dir, wo, ok), t[:, None])
        s.pdf, s.color = p, c / p[:, None]
        return s

    def sample(self, rnd, wo, active):
        k = self.mix_f(wo)
        only1, only2 = active & (k <= 0), active & (k >= 1)
        both = active & ~(k <= 0) & ~(k >= 1)
        out = Sample(self.n)
        out.merge(only1, self.m1.sample(rnd, wo, only1))
        out.merge(only2, self.m2.sample(rnd, wo, only2))
        u = rnd.next(both)
        a = both & self.tr.lt(u, 1 - k, both)
        b = both & ~a
        s = self._sample_mat(rnd, wo, a, self.m1, self.m2, k)
        out.merge(a, s)
        out.merge(a & ~s.valid, self.m2.sample(rnd, wo, a & ~s.valid))
        s = self._sample_mat(rnd, wo, b, self.m2, self.m1, 1 - k)
        out.merge(b, s)
        out.merge(b & ~s.valid, self.m1.sample(rnd, wo, b & ~s.valid))
        return out


class _PlasticDiffuse(Lambert):  # plastic.art:12-31
    def __init__(self, surf, kd, eta, tr):
        super().__init__(surf, kd, tr)
        self.eta, self.fdr = eta, fresnel_diffuse_factor(eta)

    def scattering(self, cos_i):
        return (1 - fresnel_dielectric(self.eta, cos_i)) * self.eta * self.eta / (1 - self.fdr)

    def eval(self, wi, wo, active=True):
        return Lambert.eval(self, wi, wo) * self.scattering(np.abs(dot(wi, self.L.n)))[:, None]

    def sample(self, rnd, wo, active):
        s = Lambert.sample(self, rnd, wo, active)
        s.color = s.color * self.scattering(np.abs(dot(s.dir, self.L.n)))[:, None]
        return s


def make_plastic(surf, n1, n2, kd, ks, micro, tr, mutant):  # plastic.art:2-41, PlasticBSDF.cpp:30-38
    eta = n1 / n2
    diffuse = _PlasticDiffuse(surf, kd, eta, tr)
    specular = make_conductor(surf, [0, 0, 0], [1, 1, 1], ks, micro, tr, mutant)
    n = surf.local.n
    mix_f = lambda wo: fresnel_dielectric(eta, np.abs(dot(wo, n)))
    mix_eval = (lambda wi, wo: mix_f(wi)) if mutant == "plastic_mix_at_cos_in" else None
    return VariadicMix(diffuse, specular, mix_f, tr, mix_eval)


class PureDielectric(Bsdf):  # dielectric.art:2-23
    is_specular = True

    def __init__(self, surf, n1, n2, ks, kt, tr=None):
        super().__init__(surf, tr)
        self.k = np.where(surf.entering, n1 / n2, n2 / n1)
        self.ks, self.kt = np.asarray(ks, np.float64), np.asarray(kt, np.float64)

    def sample(self, rnd, wo, active):
        n = self.L.n
        cos_o = dot(wo, n)
        some, cos_t, f = fresnel(self.k, cos_o, self.tr, active)
        cos_t, f = np.where(some, cos_t, 0.0), np.where(some, f, 1.0)
        refr = active & self.tr.gt(rnd.next(active), f, active)
        out = Sample(self.n).put(active & ~refr, reflect(wo, n), np.broadcast_to(self.ks, (self.n, 3)), 1.0)
        return out.put(refr, refract(wo, n, self.k, cos_o, cos_t), np.broadcast_to(self.kt, (self.n, 3)), 1.0, self.k)


class ThinDielectric(Bsdf):  # dielectric.art:27-47
    is_specular = True

    def __init__(self, surf, n1, n2, ks, kt, tr=None):
        super().__init__(surf, tr)
        self.k, self.ks, self.kt = n1 / n2, np.asarray(ks, np.float64), np.asarray(kt, np.float64)

    def sample(self, rnd, wo, active):
        n = self.L.n
        ft = fresnel_dielectric(self.k, np.abs(dot(wo, n)))
        f = ft + (1 - ft) * ft / (ft + 1)
        refr = active & self.tr.gt(rnd.next(active), f, active)
        out = Sample(self.n).put(active & ~refr, normalize(reflect(wo, n)), np.broadcast_to(self.ks, (self.n, 3)), 1.0)
        return out.put(refr, -wo, np.broadcast_to(self.kt, (self.n, 3)), 1.0)


def tint_color(c):  # principled.art:50-57
    lum = luminance(c)
    return c / lum if lum > FLT_EPS else np.ones(3)


def positive(v):  # shading.art:62-66
    return np.where((v[:, 2] >= 0)[:, None], v, -v)


class Principled(Bsdf):
    """make_principled_bsdf, principled.art:241-481; `m` the material record
    (alpha_u / alpha_v are compute_roughness's ax / ay, before the clamp)."""
    MICRO_EPS = GRAZING_EPS = 1e-5

    def __init__(self, surf, m, tr=None, mutant=None):
        super().__init__(surf, tr)
        self.mutant = mutant
        self.base = np.asarray(m.kd[:], np.float64)
        for k in ("ior", "diffuse_transmission", "specular_transmission", "specular_tint", "flatness", "metallic", "sheen",
                  "sheen_tint", "clearcoat", "clearcoat_gloss", "clearcoat_roughness"):
            setattr(self, k, float(getattr(m, k)))
        self.ru, self.rv = max(1e-3, float(m.alpha_u)), max(1e-3, float(m.alpha_v))  # :258-259
        self.thin, self.top_only = bool(m.thin), bool(m.clearcoat_top_only)
        inverted = (surf.entering | self.thin) if mutant != "eta_not_inverted" else np.zeros(self.n, bool)
        self.eta = np.where(inverted, 1 / self.ior, self.ior)  # :268
        self.refl_micro = Microfacet(MF_VNDF_GGX, self.ru, self.rv, mutant)  # :67-72
        f = 0.65 * self.ior - 0.35
        self.refr_micro = (Microfacet(MF_VNDF_GGX, np.clip(f * self.ru, 0, 1), np.clip(f * self.rv, 0, 1), mutant)
                           if self.thin else self.refl_micro)  # :73-80

    # -- the terms, on vectors of the shading frame (principled.art:82-194)
    def _fresnel_term(self, wi, wo, h):
        hdv, hdl = np.abs(dot(wo, h)), np.abs(dot(wi, h))
        f1 = fresnel_dielectric(self.eta, hdv)[:, None] * np.ones(3)
        a = lerp(np.ones(3), tint_color(self.base), self.specular_tint)
        r0 = lerp(a * schlick_r0(self.eta)[:, None], self.base, self.metallic)
        f2 = r0 + (1 - r0) * schlick_approx(hdl)[:, None]
        return np.where((hdv * hdl <= FLT_EPS)[:, None], 0.0, lerp(f1, f2, self.metallic))

    def _subsurface(self, wi, wo, h):
        hl = dot(wi, h)
        fss90 = hl * hl * self.ru * self.rv
        l, v = np.abs(wi[:, 2]), np.abs(wo[:, 2])
        lk, vk = schlick_approx(l), schlick_approx(v)
        fss = (1 - lk + fss90 * lk) * (1 - vk + fss90 * vk)
        return 1.25 * (fss * (1 / (l + v + 1e-5) - 0.5) + 0.5)

    def _sheen(self, wi):
        l = np.abs(wi[:, 2])
        tint = self.base if self.mutant == "sheen_base_color" else tint_color(self.base)
        return col(lerp(np.ones(3), tint, self.sheen_tint), self.sheen * schlick_approx(l) * l)

    def _diffuse(self, wi, wo, h):
        l, v = np.abs(wi[:, 2]), np.abs(wo[:, 2])
        lk, vk = schlick_approx(l), schlick_approx(v)
        diff = (1 - 0.5 * lk) * (1 - 0.5 * vk)
        rr = (np.abs(dot(wi, wo)) + 1) * (self.ru + self.rv) / 2
        retro = rr * (lk + vk + lk * vk * (rr - 1))
        ss = 1 - self.flatness + self._subsurface(wi, wo, h) * self.flatness if self.thin else 1.0
        return (1 / PI) * (diff + retro) * ss * l

    def _translucent(self, wi, wo):
        l, v = np.abs(wi[:, 2]), np.abs(wo[:, 2])
        return (1 / PI) * (1 - 0.5 * schlick_approx(l)) * (1 - 0.5 * schlick_approx(v)) * l

    def _reflection(self, wi, wo, h):
        mi = self.refl_micro
        return col(self._fresnel_term(wi, wo, h), np.abs(mi.D(h) * mi.G(wi, wo, h) * reflective_jacobian(wo[:, 2])))

    def _refraction(self, wi, wo, h):
        if self.thin:
            ft = fresnel_dielectric(self.eta, np.abs(wo[:, 2]))
            return col(np.sqrt(self.base), 1 - (ft + (1 - ft) * ft / (ft + 1)))
        mi = self.refr_micro
        hdi, hdo = dot(wi, h), dot(wo, h)
        f = fresnel_dielectric(self.eta, np.abs(hdo))
        jac = refractive_jacobian(self.eta, hdi, hdo, self.mutant)
        norm = np.abs(safe_div(hdo * jac, wo[:, 2]))
        return col(self.base, (1 - f) * mi.D(h) * mi.G(wi, wo, h) * norm)

    def _clearcoat(self, wi, wo, h):
        r = 0.25
        r2 = max(0.001, self.clearcoat_roughness * (1 - self.clearcoat_gloss) + 0.01 * self.clearcoat_gloss)
        f = 0.04 + (1 - 0.04) * schlick_approx(np.abs(dot(wi, h)))
        g = g_1_smith(wi, r, r) * g_1_smith(wo, r, r)
        return np.abs(r * ndf_ggx(h, r2, r2) * f * g * reflective_jacobian(wo[:, 2]) * wi[:, 2])[:, None] * np.ones(3)

    def _lobes(self, wo):  # calcLobeDistribution, principled.art:203-236
        metallic, dt_in, st_in = (np.clip(v, 0, 1) for v in (self.metallic, self.diffuse_transmission, self.specular_transmission))
        abs_gen = luminance(self.base)
        abs_spec = lerp(1.0, luminance(tint_color(self.base)), self.specular_tint)
        diff_refl = np.clip(abs_gen * (1 - metallic) * (1 - st_in), 0, 1) * np.ones(self.n)
        f = fresnel_dielectric(self.eta, np.abs(wo[:, 2]))
        spec_refl = np.clip(abs_spec * (1 - f) + f, 0, 1)
        if dt_in > 0 or st_in > 0:
            diff_trans = np.clip(abs_gen * dt_in * diff_refl, 0, 1)
            spec_trans = np.clip((1 - f) * abs_gen * (1 - metallic) * st_in, 0, 1)
        else:
            diff_trans = spec_trans = np.zeros(self.n)
        norm = diff_refl + spec_refl + diff_trans + spec_trans
        none = norm <= FLT_EPS
        return [np.where(none, d, v / norm) for d, v in ((1.0, diff_refl), (0.0, diff_trans), (0.0, spec_refl), (0.0, spec_trans))]

    def _same_hemisphere(self, a, b, active=True):
        self.tr.ge(a[:, 2], 0.0, active)
        self.tr.ge(b[:, 2], 0.0, active)
        return (a[:, 2] >= 0) == (b[:, 2] >= 0)

    def eval(self, wi_w, wo_w, active=True):  # :271-338
        wo, wi = self.L.to_local(wo_w), self.L.to_local(wi_w)
        trans = ~self._same_hemisphere(wi, wo, active)
        h = np.where(trans[:, None], halfway_refractive(wi, wo, self.eta), halfway(wi, wo))
        h = np.where(((h[:, 2] >= 0) == (wo[:, 2] >= 0))[:, None], h, -h)
        upper = (self.surf.entering == (wi[:, 2] >= 0)) & (self.surf.entering == (wo[:, 2] >= 0))
        black = self.tr.le(np.abs(wi[:, 2]), self.GRAZING_EPS, active)
        metallic, st = np.clip(self.metallic, 0, 1), np.clip(self.specular_transmission, 0, 1)
        dw = (1.0 if self.thin else 1 - metallic) * (1 - st)
        tw = (1 - metallic) * st
        refl = np.zeros((self.n, 3))
        if dw > 0:
            refl = refl + col(self.base, self._diffuse(wi, wo, h) * dw)
        if self.sheen > 0:
            refl = refl + self._sheen(wi) * dw
        refl = refl + self._reflection(wi, wo, h)
        if self.clearcoat > 0:
            cc = self._clearcoat(wi, wo, h) * self.clearcoat
            refl = refl + (np.where(upper[:, None], cc, 0.0) if self.top_only else cc)
        tra = np.zeros((self.n, 3))
        if self.thin and self.diffuse_transmission > 0:
            tra = tra + col(self.base, self._translucent(wi, wo) * self.diffuse_transmission)
        if self.specular_transmission > 0:
            tra = tra + self._refraction(wi, wo, h) * tw
        return np.where(black[:, None], 0.0, np.where(trans[:, None], tra, refl))

    def _bound(self, v):
        return np.where(v <= self.MICRO_EPS, 0.0, v)

    def _spec_refl_pdf(self, wo, wi):  # :344-352
        pwo, pwi = positive(wo), positive(wi)
        h = halfway(pwo, pwi)
        return np.abs(self._bound(self.refl_micro.pdf(pwi, pwo, h)) * reflective_jacobian(dot(pwo, h)))

    def _spec_trans_pdf(self, wo, wi):  # :354-363
        pwo, pwi = positive(wo), -positive(wi)
        h = halfway_refractive(pwi, pwo, self.eta)
        jac = refractive_jacobian(self.eta, dot(pwi, h), dot(pwo, h), self.mutant)
        return np.abs(self._bound(self.refr_micro.pdf(pwi, pwo, h)) * jac)

    def pdf(self, wi_w, wo_w, active=True):  # :365-381
        wo, wi = self.L.to_local(wo_w), self.L.to_local(wi_w)
        zero = self.tr.le(np.abs(wo[:, 2]), self.GRAZING_EPS, active) | self.tr.le(np.abs(wi[:, 2]), self.GRAZING_EPS, active)
        dr, dt, sr, st = self._lobes(wo)
        dp = np.abs(wi[:, 2]) / PI
        same = self._same_hemisphere(wo, wi, active)
        through = dt * dp + (st if self.thin else st * self._spec_trans_pdf(wo, wi))
        return np.where(zero, 0.0, np.where(same, dr * dp + sr * self._spec_refl_pdf(wo, wi), through))

    def _micro_half(self, micro, rnd, pwo, active):
        m, mpdf = micro.sample(rnd, pwo, active, self.tr)
        ok = active & ~(self.tr.le(mpdf, self.MICRO_EPS, active) | (dot(m, m) <= FLT_EPS))
        oh = normalize(m)
        h = np.where(self.tr.lt(dot(oh, pwo), 0.0, ok)[:, None], -oh, oh)
        return h, mpdf, ok

    def sample(self, rnd, wo_w, active):  # :386-479
        tr = self.tr
        wo = self.L.to_local(wo_w)
        active = active & ~tr.le(np.abs(wo[:, 2]), self.GRAZING_EPS, active)
        dr, dt, sr, st = self._lobes(wo)
        pick = rnd.next(active)
        is_dr = active & tr.lt(pick, dr, active)
        is_dt = active & ~is_dr & tr.lt(pick, dr + dt, active & ~is_dr)
        is_st = active & ~is_dr & ~is_dt & tr.lt(pick, dr + dt + st, active & ~is_dr & ~is_dt)
        is_sr = active & ~is_dr & ~is_dt & ~is_st
        same_as_wo = lambda v: np.where(((wo[:, 2] >= 0) == (v[:, 2] >= 0))[:, None], v, -v)
        dirs, pdfs, ok = np.zeros((self.n, 3)), np.zeros(self.n), np.zeros(self.n, bool)

        def put(mask, d, p):
            nonlocal dirs, pdfs, ok
            dirs, pdfs, ok = np.where(mask[:, None], d, dirs), np.where(mask, p, pdfs), ok | mask

        diff = is_dr | is_dt
        d, dpdf = sample_cosine_hemisphere(rnd.next(diff), rnd.next(diff))
        wi = same_as_wo(d)
        put(is_dr, wi, dpdf * dr + self._spec_refl_pdf(wo, wi) * sr)
        put(is_dt, -wi, dpdf * dt + self._spec_trans_pdf(wo, -wi) * st)
        pwo = positive(wo)
        if self.thin:
            put(is_st, -wo, st)
        elif is_st.any():
            h, mpdf, good = self._micro_half(self.refr_micro, rnd, pwo, is_st)
            cho = dot(pwo, h)
            some, cos_t, _ = fresnel(self.eta, cho, tr, good)
            pwi = normalize(refract(pwo, h, self.eta, cho, cos_t))
            through = good & some & ~self._same_hemisphere(pwo, pwi, good & some) & tr.gt(cho, FLT_EPS, good & some) \
                & tr.gt(-pwi[:, 2], self.GRAZING_EPS, good & some)
            wi = -same_as_wo(pwi)
            jac = refractive_jacobian(self.eta, dot(pwi, h), cho, self.mutant)
            put(through, wi, np.abs(mpdf * jac) * st + (np.abs(wi[:, 2]) / PI) * dt)
            pwr = normalize(reflect(pwo, h))
            tir = good & ~some
            back = tir & self._same_hemisphere(pwo, pwr, tir) & tr.gt(cho, FLT_EPS, tir) & tr.gt(pwr[:, 2], self.GRAZING_EPS, tir)
            wi = same_as_wo(pwr)
            put(back, wi, mpdf * reflective_jacobian(cho) * st + (np.abs(wi[:, 2]) / PI) * dt)
        h, mpdf, good = self._micro_half(self.refl_micro, rnd, pwo, is_sr)
        cho = dot(pwo, h)
        pwi = normalize(reflect(pwo, h))
        good = good & self._same_hemisphere(pwo, pwi, good) & tr.gt(cho, FLT_EPS, good) & tr.gt(pwi[:, 2], self.GRAZING_EPS, good)
        wi = same_as_wo(pwi)
        put(good, wi, np.abs(mpdf * reflective_jacobian(cho)) * sr + (np.abs(wi[:, 2]) / PI) * dr)
        ok = ok & ~tr.le(pdfs, FLT_EPS, ok)
        same = (wo[:, 2] >= 0) == (dirs[:, 2] >= 0)
        s_eta = np.ones(self.n) if self.thin else np.where(same, 1.0, self.eta)
        in_w = self.L.to_world(dirs)
        return Sample(self.n).put(ok, in_w, self.eval(in_w, wo_w, ok) / pdfs[:, None], pdfs, s_eta)


def make_bsdf(m, surf, tr=None, mutant=None):
    """The BSDF the reference's loader builds for material record `m` (an
    igx_material): DiffuseBSDF.cpp:22-24, ConductorBSDF.cpp:26-31,
    PlasticBSDF.cpp:30-38, DielectricBSDF.cpp:31-38, PrincipledBSDF.cpp:44-68;
    alpha_u / alpha_v are already through compute_explicit (BSDF.cpp:53-99)."""
    tr = tr if tr is not None else Trace(len(surf.entering))
    t = m.bsdf_type
    if t == DIFFUSE:  # make_diffuse_bsdf, diffuse.art:41-47
        if m.diffuse_alpha <= FLT_EPS:
            return Lambert(surf, m.kd[:], tr)
        return OrenNayar(surf, float(m.diffuse_alpha), m.kd[:], tr, mutant)
    if t == PRINCIPLED:
        return Principled(surf, m, tr, mutant)
    micro = Microfacet(m.distribution, m.alpha_u, m.alpha_v, mutant)
    if t == CONDUCTOR:
        return make_conductor(surf, m.eta[:], m.kappa[:], m.ks[:], micro, tr, mutant)
    if t == PLASTIC:
        return make_plastic(surf, float(m.ext_ior), float(m.int_ior), m.kd[:], m.ks[:], micro, tr, mutant)
    if t == DIELECTRIC:  # make_dielectric_bsdf, dielectric.art:178-189 (delta only)
        assert micro.is_delta
        cls = ThinDielectric if m.thin else PureDielectric
        return cls(surf, float(m.ext_ior), float(m.int_ior), m.ks[:], m.kt[:], tr)
    raise ValueError(t)


# ---- what the path tracer does around the BSDF (technique/pathtracer.art) -------------------
ENV_SAMPLE_DRAWS = 2       # sample_equal_area_sphere, light/env.art:82-86
UNIFORM_SELECTOR_DRAWS = 0  # make_uniform_light_selector with one light draws nothing
ENV_PDF = 1 / (4 * PI)     # equal_area_sphere_pdf, core/sampling.art:39,51


def point_light_term(position, intensity, point):
    """make_point_light.sample_direct (light/point.art:3-8) through on_shadow
    (pathtracer.art:77-94): direction, and intensity * pdf.value / pdf_l_s =
    intensity / dist^2 (an area pdf of 1 as solid angle is dist^2 / cos, cos 1)."""
    d = np.asarray(position, np.float64) - point
    dist = np.sqrt(dot(d, d))
    return d * safe_div(1.0, dist)[:, None], np.asarray(intensity, np.float64) / (dist * dist)[:, None]


def russian_roulette_pbrt(c, clamp=0.95):  # pathtracer.art:5
    return np.clip(c.max(axis=-1), 0.05, clamp)


class Replay:
    """One ray-list render of depth 2 on a single flat face, in float64: ray i
    meets the plane (normal, through plane_point) at its hit point, NEE runs
    first, then the bounce, whose ray leaves the scene."""

    def __init__(self, material, normal, plane_point, rays, draws, mutant=None):
        rays = np.asarray(rays, np.float64)
        self.org, self.dir = rays[:, 0:3], rays[:, 3:6]
        normal = np.asarray(normal, np.float64)
        t = dot(np.asarray(plane_point, np.float64) - self.org, normal) / dot(self.dir, normal)
        self.point = self.org + self.dir * t[:, None]
        self.n = len(rays)
        self.tr = Trace(self.n)
        self.surf = Surface(normal, self.dir, self.point)
        self.bsdf = make_bsdf(material, self.surf, self.tr, mutant)
        self.out = -self.dir
        self.draws = draws
        self.all = np.ones(self.n, bool)

    @property
    def stable(self):
        return ~self.tr.unstable

    @property
    def ill(self):
        return self.tr.ill

    def eval_point_light(self, position, intensity):
        """Observable (a): the film under one point light, NEE only
        (pathtracer.art:86-97: a delta light has MIS weight 1)."""
        wi, term = point_light_term(position, intensity, self.point)
        return self.bsdf.eval(wi, self.out) * term

    def env_nee(self, radiance=1.0, min_depth=2):
        """Observable (b) under a constant environment with NEE: ("NEE Weights",
        "Direct Weights"), pathtracer.art:72-97, 152-153, 178-186."""
        rnd = Draws(self.draws)
        wi = equal_area_square_to_sphere(rnd.next(), rnd.next())
        pdf_e = self.bsdf.pdf(wi, self.out)
        nee = self.bsdf.eval(wi, self.out) * (radiance / ENV_PDF / (1 + pdf_e / ENV_PDF))[:, None]
        s, rr = self._bounce(rnd, min_depth)
        direct = np.where(s.valid[:, None], s.color * (radiance / rr / (1 + (1 / s.pdf) * ENV_PDF))[:, None], 0.0)
        return nee, direct

    def _bounce(self, rnd, min_depth):
        s = self.bsdf.sample(rnd, self.out, self.all)
        rr = russian_roulette_pbrt(s.color) if 2 > min_depth else np.ones(self.n)  # depth 1: pt.depth + 1 > min_path_len
        s.valid = s.valid & ~self.tr.ge(rnd.next(s.valid), rr, s.valid)  # a killed path contributes nothing
        return s, rr

    def sampled(self, min_depth=2):
        """Observable (c), without NEE: the bounce's (direction, weight / rr, valid, eta, pdf)."""
        s, rr = self._bounce(Draws(self.draws), min_depth)
        return s.dir, s.color / rr[:, None], s.valid, s.eta, s.pdf


# ---- the comparison ---------------------------------------------------------------------------
def deviation(got, want, stable):
    """max |got - want| / max(|want|, floor) over the stable rays; the floor is
    1e-3 of the case's 90th-percentile |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    g, w = got[stable], want[stable]
    if not w.size:
        return 0.0
    if not np.isfinite(g).all():
        return math.inf
    floor = max(1e-3 * np.percentile(np.abs(w), 90), 1e-30)
    return float((np.abs(g - w) / np.maximum(np.abs(w), floor)).max())


def check(got, want, stable, allowed):
    """(passes, deviation): used for the device, the oracle and the mutants alike."""
    dev = deviation(got, want, stable)
    return dev <= allowed, dev

"""The measured fenestration BSDFs in numpy float64, vectorised over rays,
written from the reference's artic text (bsdf/tensortree.art, bsdf/klems.art,
core/warp.art:24-48, core/interval.art) in the manner of tests/bsdf_ref.py.

The tables are read from an igx_measured record (include/igx_scene.h), whose
layout tests/test_measured_loader.py pins against hand-derived values.  Every
grid decision (p >= 1), hemisphere test, theta and phi binning and the three
thresholds go through bsdf_ref.Trace, so rays within 1e-5 of a cell boundary
are marked unstable.

One deliberate deviation from the artic text, shared with the device: every
tree coordinate is brought into [0, 1) before it forms an index
(concentric_disk_to_square can return exactly 1, which in the reference reads
one value past the leaf).

`mutant=` swaps in one deliberate porting slip (MUTANTS)."""
import math

import numpy as np

import bsdf_ref as B

FLT_EPS, PI = B.FLT_EPS, B.PI
TENSORTREE, KLEMS = 5, 6  # igx_material.bsdf_type
FR, FT, BR, BT = range(4)  # igx_measured.component
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))  # the device clamps to the largest float below 1

MUTANTS = ("in_out_exchanged", "transmission_exchanged", "leaf_bits_reversed", "klems_row_col_exchanged",
           "k_fi_without_flip", "third_draw_unconditional")


class Component:
    """One igx_measured_component and its words."""

    def __init__(self, measured, k):
        c = measured.component[k]
        words = np.ctypeslib.as_array(measured.words, (measured.num_words,)).copy() if measured.num_words else np.zeros(0, np.uint32)
        w = words[c.offset:]
        self.total = float(c.total)
        if measured.kind == 0:
            self.ndim, self.root_is_leaf, self.max_depth = int(c.ndim), bool(c.root_is_leaf), int(c.max_depth)
            self.nodes = w[:c.node_count].view(np.int32).astype(np.int64)
            self.raw_values = w[c.node_count:c.node_count + c.value_count].view(np.float32)
            self.single = np.signbit(self.raw_values)
            self.values = self.raw_values.astype(np.float64)
        else:
            rt, ct = int(c.theta_count[0]), int(c.theta_count[1])
            self.rows, self.cols = int(c.entry_count[0]), int(c.entry_count[1])
            self.basis = []
            at = 0
            for tc in (rt, ct):
                rec = w[at:at + 4 * tc].reshape(tc, 4)
                self.basis.append(dict(lower=rec[:, 1].copy().view(np.float32).astype(np.float64),
                                       upper=rec[:, 2].copy().view(np.float32).astype(np.float64),
                                       phis=rec[:, 3].astype(np.int64), first=w[at + 4 * tc:at + 5 * tc].astype(np.int64)))
                at += 5 * tc
            self.matrix = w[at:at + self.rows * self.cols].view(np.float32).astype(np.float64).reshape(self.rows, self.cols)


# ---- core/warp.art -------------------------------------------------------------------------
def prodsign(x, y):  # common.art:93
    return np.where(np.signbit(y), -x, x)


def concentric_disk_to_square(px, py, tr, active):  # warp.art:24-40
    quadrant = tr.gt(np.abs(px), np.abs(py), active)
    r_sign = np.where(quadrant, px, py)
    r = np.copysign(np.sqrt(px * px + py * py), r_sign)
    phi = np.arctan2(prodsign(py, r_sign), prodsign(px, r_sign))
    c = 4 * phi / PI
    t = np.where(quadrant, c, 2 - c) * r
    return (np.where(quadrant, r, t) + 1) * 0.5, (np.where(quadrant, t, r) + 1) * 0.5


def spherical_from_dir(d):  # warp.art:44-48
    theta = np.arccos(np.clip(d[:, 2], -1, 1))
    phi = np.arctan2(d[:, 1], d[:, 0])
    return theta, np.where(phi < 0, phi + 2 * PI, phi)


def unit(p):
    return np.minimum(np.maximum(p, 0.0), BELOW_ONE)


# ---- bsdf/tensortree.art ---------------------------------------------------------------------
def tt_eval_component(comp, in_dir, out_dir, tr, active, mutant=None):  # :80-114
    n = len(in_dir)
    active = np.broadcast_to(active, (n,))
    ox, oy = concentric_disk_to_square(out_dir[:, 0], out_dir[:, 1], tr, active)
    if comp.ndim == 3:
        in_t = (0.5 - FLT_EPS) - 0.5 * np.sqrt(in_dir[:, 0] ** 2 + in_dir[:, 1] ** 2)
        pos = [in_t, ox, oy]
    else:
        ix, iy = concentric_disk_to_square(-in_dir[:, 0], -in_dir[:, 1], tr, active)
        pos = [ix, iy, ox, oy]
    pos = [unit(p) for p in pos]
    nd = comp.ndim
    leaf = np.zeros(n, np.int64)
    if not comp.root_is_leaf:  # tt_climb_tree :67-77 with tt_lookup_grid :38-49
        node = np.zeros(n, np.int64)
        climbing = active.copy()
        for _ in range(comp.max_depth):
            child = np.zeros(n, np.int64)
            for i in range(nd - 1, -1, -1):
                p = 2 * pos[i]
                t = tr.ge(p, 1.0, climbing)
                child |= t.astype(np.int64) << i
                pos[i] = np.where(climbing, p - t, pos[i])
            nxt = comp.nodes[np.where(climbing, node + child, 0)]
            node = np.where(climbing, nxt, node)
            climbing = climbing & (node >= 0)
        assert not climbing.any()
        leaf = np.where(active, -node - 1, 0)
    single = comp.single[leaf]
    # tt_lookup_leaf :52-64: the last coordinate is the lowest bit
    off = np.zeros(n, np.int64)
    for k, i in enumerate(range(nd - 1, -1, -1)):
        p = 2 * pos[i]
        bit = tr.ge(p, 1.0, active & ~single).astype(np.int64)  # (scale * pos) as i32
        off += bit << ((nd - 1 - k) if mutant == "leaf_bits_reversed" else k)
    full = comp.values[np.where(single, leaf, np.minimum(leaf + off, len(comp.values) - 1))]
    return np.where(active, np.where(single, -comp.values[leaf], full), 0.0)


def positive(v):
    return np.where((v[:, 2] >= 0)[:, None], v, -v)


def tensortree_eval(comps, wi, wo, tr, active, mutant=None):  # :146-165
    n = len(wi)
    active = np.broadcast_to(active, (n,)).copy()
    dark = tr.le(np.abs(wi[:, 2]), FLT_EPS, active) | tr.le(np.abs(wo[:, 2]), FLT_EPS, active)
    active &= ~dark
    in_front, out_front = tr.ge(wi[:, 2], 0.0, active), tr.ge(wo[:, 2], 0.0, active)
    pwi, pwo = positive(wi), positive(wo)
    ft, bt = (BT, FT) if mutant == "transmission_exchanged" else (FT, BT)
    calls = [(in_front & out_front, FR, pwo, pwi), (in_front & ~out_front, ft, pwi, -pwo),
             (~in_front & out_front, bt, pwo, -pwi), (~in_front & ~out_front, BR, -pwo, -pwi)]
    factor = np.zeros(n)
    for mask, k, a, b in calls:
        m = mask & active
        if comps[k].total > 0 and m.any():
            if mutant == "in_out_exchanged" and k == FR:
                a, b = b, a
            factor = np.where(m, tt_eval_component(comps[k], a, b, tr, m, mutant), factor)
    return factor * np.abs(wi[:, 2])


# ---- bsdf/klems.art ----------------------------------------------------------------------------
def k_index_of(basis, d, tr, active):  # :49-67
    theta, phi = spherical_from_dir(d)
    lower, count = basis["lower"], len(basis["lower"])
    # interval::binary_search(count, lower[k] < theta): the bands are ascending, so the
    # search ends behind the last band whose lower bound is below theta; then its clamp
    below = np.zeros((len(d), count), bool)
    for k in range(count):
        below[:, k] = tr.lt(lower[k], theta, active)
    first = np.zeros(len(d), np.int64)
    length = np.full(len(d), count, np.int64)
    while (length > 0).any():
        go = length > 0
        half = length // 2
        middle = np.minimum(first + half, count - 1)
        pred = below[np.arange(len(d)), middle]
        first = np.where(go & pred, middle + 1, first)
        length = np.where(go, np.where(pred, length - (half + 1), half), length)
    i = np.clip(first - 1, 0, count - 1)
    phis = basis["phis"][i]
    x = phi * phis * (1 / PI) / 2 + 0.5
    tr._note(x, np.round(x), np.broadcast_to(active, x.shape))  # `as i32` steps at every integer
    j = np.maximum(0, np.trunc(x).astype(np.int64))
    j = np.where(j >= phis, 0, j)
    return basis["first"][i] + j


def k_eval_component(comp, in_dir, out_dir, tr, active, mutant=None):  # :72-78
    in_idx = k_index_of(comp.basis[1], in_dir, tr, active)
    out_idx = k_index_of(comp.basis[0], out_dir, tr, active)
    if mutant == "klems_row_col_exchanged":
        return np.where(active, comp.matrix[np.minimum(in_idx, comp.rows - 1), np.minimum(out_idx, comp.cols - 1)], 0.0)
    return np.where(active, comp.matrix[out_idx, in_idx], 0.0)


def klems_eval(comps, wi, wo, tr, active, mutant=None):  # :189-202
    n = len(wi)
    active = np.broadcast_to(active, (n,))
    in_front, out_front = tr.ge(wi[:, 2], 0.0, active), tr.ge(wo[:, 2], 0.0, active)
    flip = np.array([-1.0, -1.0, 1.0])
    k_fi = (lambda v: v) if mutant == "k_fi_without_flip" else (lambda v: v * flip)
    k_bo = lambda v: v * np.array([1.0, 1.0, -1.0])  # noqa: E731
    ft, bt = (BT, FT) if mutant == "transmission_exchanged" else (FT, BT)
    calls = [(in_front & out_front, FR, k_fi(wo), wi), (in_front & ~out_front, ft, wi, -wo),
             (~in_front & out_front, bt, -wi, wo), (~in_front & ~out_front, BR, -wo, k_bo(wi))]
    factor = np.zeros(n)
    for mask, k, a, b in calls:
        m = mask & active
        if comps[k].total > 0 and m.any():
            if mutant == "in_out_exchanged" and k == FR:
                a, b = b, a
            factor = np.where(m, k_eval_component(comps[k], a, b, tr, m, mutant), factor)
    return factor * np.abs(wi[:, 2])


# ---- make_tensortree_bsdf :181-238, make_klems_bsdf :170-280 -----------------------------------
def tt_transform_matrix(normal, up):  # tensortree.art:169-177: columns right, nup, normal, as they come
    right = np.cross(up, normal)
    ident = B.dot(right, right) <= FLT_EPS
    eye = np.eye(3)
    cols = [np.where(ident[:, None], eye[k], c) for k, c in enumerate((right, np.cross(normal, right), normal))]
    return cols, ident


class Measured(B.Bsdf):
    def __init__(self, surf, material, measured, tr=None, mutant=None):
        super().__init__(surf, tr)
        self.kind = material.bsdf_type
        self.color = np.array(material.kd[:], np.float64)
        self.comps = [Component(measured, k) for k in range(4)]
        self.mutant = mutant
        fr, ft, br, bt = (np.float32(c.total) for c in self.comps)
        sdiv = lambda a, b: float(np.float32(0) if abs(b) <= FLT_EPS else a / b)  # noqa: E731  (safe_div, in float as the host)
        self.front_refl_prob, self.back_refl_prob = sdiv(fr, fr + bt), sdiv(br, br + ft)
        n = np.where(surf.entering[:, None], surf.local.n, -surf.local.n)  # the normal without the flip
        up = np.broadcast_to(np.array(material.up[:], np.float64), n.shape)
        self.cols, self.identity = tt_transform_matrix(n, up)

    def to_local(self, v):
        return B.vec(B.dot(self.cols[0], v), B.dot(self.cols[1], v), B.dot(self.cols[2], v))

    def to_world(self, v):
        return self.cols[0] * v[:, 0:1] + self.cols[1] * v[:, 1:2] + self.cols[2] * v[:, 2:3]

    def local_eval(self, wi, wo, active):
        f = klems_eval if self.kind == KLEMS else tensortree_eval
        return f(self.comps, wi, wo, self.tr, active, self.mutant)

    def eval(self, wi, wo, active=True):
        return B.col(self.color, self.local_eval(self.to_local(wi), self.to_local(wo), active))

    def _refl_prob(self, wo, active):
        return np.where(self.tr.ge(wo[:, 2], 0.0, active), self.front_refl_prob, self.back_refl_prob)

    def pdf(self, wi, wo, active=True):
        wo, wi = self.to_local(wo), self.to_local(wi)
        refl_prob = self._refl_prob(wo, active)
        same = self.tr.ge(wo[:, 2], 0.0, active) == self.tr.ge(wi[:, 2], 0.0, active)
        return np.where(same, refl_prob, 1 - refl_prob) * (np.abs(wi[:, 2]) / PI)

    def sample(self, rnd, wo, active):
        wo = self.to_local(wo)
        d, cpdf = B.sample_cosine_hemisphere(rnd.next(active), rnd.next(active))
        live = active & ~self.tr.le(cpdf, FLT_EPS, active)
        refl_prob = self._refl_prob(wo, live)
        third = live if self.mutant == "third_draw_unconditional" else live & (refl_prob > 0)
        u = rnd.next(third)
        refl = (refl_prob > 0) & self.tr.lt(u, refl_prob, third)
        same = np.where(((wo[:, 2] >= 0) == (d[:, 2] >= 0))[:, None], d, -d)  # make_same_hemisphere(wo, dir)
        wi = np.where(refl[:, None], same, -same)
        e_pdf = np.where(refl, refl_prob, 1 - refl_prob) * cpdf
        live = live & ~self.tr.le(e_pdf, FLT_EPS, live)
        weight = B.col(self.color, self.local_eval(wi, wo, live) / np.where(live, e_pdf, 1.0))
        return B.Sample(self.n).put(live, self.to_world(wi), weight, e_pdf)


class Replay(B.Replay):
    """bsdf_ref.Replay on a measured material: `desc` is the scene's igx_scene_desc."""

    def __init__(self, desc, normal, plane_point, rays, draws, mutant=None):
        rays = np.asarray(rays, np.float64)
        self.org, self.dir = rays[:, 0:3], rays[:, 3:6]
        normal = np.asarray(normal, np.float64)
        t = B.dot(np.asarray(plane_point, np.float64) - self.org, normal) / B.dot(self.dir, normal)
        self.point = self.org + self.dir * t[:, None]
        self.n = len(rays)
        self.tr = B.Trace(self.n)
        self.surf = B.Surface(normal, self.dir, self.point)
        material = desc.materials[desc.entities[0].material]
        self.bsdf = Measured(self.surf, material, desc.measured[material.measured], self.tr, mutant)
        self.out = -self.dir
        self.draws = draws
        self.all = np.ones(self.n, bool)


# ---- integrals for the known answers and the expected images -----------------------------------
def hemisphere_grid(n_theta=256, n_phi=512):
    """Midpoint directions of the upper hemisphere and their projected weights cos * d omega."""
    ct = (np.arange(n_theta) + 0.5) / n_theta  # uniform in cos^2 is exact for cos-weighted constants
    mu = np.sqrt(ct)
    phi = (np.arange(n_phi) + 0.5) / n_phi * 2 * PI
    M, P = np.meshgrid(mu, phi, indexing="ij")
    s = np.sqrt(1 - M * M)
    d = B.vec(s * np.cos(P), s * np.sin(P), M).reshape(-1, 3)
    return d, np.full(len(d), PI / (n_theta * n_phi))  # cos d omega = d(cos^2)/2 d phi

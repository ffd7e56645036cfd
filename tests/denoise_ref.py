"""tests/denoise_ref.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restatement of the a-trous denoiser (hrt_denoise), written from the contract in include/hip_raytrace.h ("The filter") alone: numpy
float32, one elementary operation per numpy call, in the statement order of the contract.  Every tap is evaluated for the whole image
at once (a shifted view per tap), which keeps each pixel's own order: dy outer, dx inner, multiply then add.  Nothing of
ilgpu_raytracing_amd/csrc is imported.  `exp_fn` and `fmax_fn` are the shared functions of include/hrt_math.h, taken from the oracle
(orc.math_eval) the way oracle/orc_indep.py takes the shared sin / cos; `pack_fn` is the oracle's PackRGBA8.
"""
import numpy as np

f32 = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)      # exact in float32, and so is every product of two


def defaults(iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0):
    """The parameter rules of hrt_denoise_params: 0 iterations select 5, a sigma <= 0 its default; a NaN goes through."""
    it = 5 if iterations == 0 else iterations
    sc = f32(4.0) if sigma_color <= 0 else f32(sigma_color)
    sn = f32(0.5) if sigma_normal <= 0 else f32(sigma_normal)
    sp = f32(0.02) if sigma_plane <= 0 else f32(sigma_plane)
    return it, sc, sn, sp


def make_fns(orc):
    exp_fn = lambda x: orc.math_eval("exp", x).reshape(np.shape(x))
    fmax_fn = lambda a, b: orc.math_eval("fmax", a, np.broadcast_to(f32(b), np.shape(a))).reshape(np.shape(a))

    def pack_fn(rgb):
        rgb = np.asarray(rgb, np.float32).reshape(-1, 3)
        L = orc.lib()
        return np.array([L.orc_pack_rgba8(float(r), float(g), float(b)) for r, g, b in rgb], np.int64).astype(np.int32)
    return exp_fn, fmax_fn, pack_fn


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, else `fill`."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -dy), min(h, h - dy)
    xs0, xs1 = max(0, -dx), min(w, w - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return out


class SeamTaps:
    """Test-only diagnostic, no part of the filter: which far taps counted.  The device kernels give every 32x8 tile of one
    sub-lattice of step s (pixels with equal x mod s, y mod s) to a workgroup (tests/denoise_tiles.py); a tap of the outer ring
    (|dx| == 2 or |dy| == 2) of a pixel near a tile border reads a record of the neighbour tile.  Per pass and axis this counts the
    hit pixels that have such a tap inside the image (`could`) and those for which at least one of them was taken, w > 0 (`took`).
    passes: one dict(step=s, x=(took, could), y=(took, could)) per a-trous pass, in order."""

    def __init__(self):
        self.passes = []

    def begin(self, width, height, s, hit):
        from tests.denoise_tiles import TILE_W, TILE_H
        self.s, self.hit, self.size = s, hit, (width, height)
        self.y, self.x = np.mgrid[0:height, 0:width]
        self.tile = {"x": (self.x // s, TILE_W), "y": (self.y // s, TILE_H)}          # lattice coordinate u = x div s, tile = u div 32
        self.took = {a: np.zeros((height, width), bool) for a in "xy"}
        self.could = {a: np.zeros((height, width), bool) for a in "xy"}

    def tap(self, dx, dy, take):
        if max(abs(dx), abs(dy)) != 2:
            return
        w, h = self.size
        qx, qy = self.x + dx * self.s, self.y + dy * self.s
        inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        for a, d in (("x", dx), ("y", dy)):
            u, t = self.tile[a]
            other = self.hit & inside & ((u + d) // t != u // t)
            self.could[a] |= other
            self.took[a] |= other & take

    def end(self):
        self.passes.append(dict(step=self.s, **{a: (int(self.took[a].sum()), int(self.could[a].sum())) for a in "xy"}))


def denoise(frame, width, height, fns, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0, demodulate=True, pack=True,
            seam_taps=None):
    """frame: dict with radiance, gb_normalWS, gb_worldPos, gb_baseColor (n, 3) float32, depth (n,) float32, gb_hitMask (n,) int32.
    Returns (denoised radiance (n, 3) float32, denoised colour (n,) int32 or None).  seam_taps: an optional SeamTaps to fill."""
    exp_fn, fmax_fn, pack_fn = fns
    it, sc0, sn, sp = defaults(iterations, sigma_color, sigma_normal, sigma_plane)
    W, Hh = width, height
    rad = np.asarray(frame["radiance"], np.float32).reshape(Hh, W, 3)
    n = np.asarray(frame["gb_normalWS"], np.float32).reshape(Hh, W, 3)
    P = np.asarray(frame["gb_worldPos"], np.float32).reshape(Hh, W, 3)
    base = np.asarray(frame["gb_baseColor"], np.float32).reshape(Hh, W, 3)
    depth = np.asarray(frame["depth"], np.float32).reshape(Hh, W)
    hit = np.asarray(frame["gb_hitMask"]).reshape(Hh, W) != 0
    with np.errstate(all="ignore"):
        # 1. prepare
        a = np.ones((Hh, W, 3), np.float32)
        if demodulate:
            a = np.where(hit[..., None], fmax_fn(base, 0.01), a).astype(np.float32)
        c = rad / a
        kx = f32(1.0) / ((sp * sp) * fmax_fn(depth * depth, 1e-12))
        kn = f32(1.0) / (sn * sn)
        # 2. iterations
        for i in range(it):
            s = 1 << i
            sc = sc0 * f32(2.0 ** -i)
            kc = f32(1.0) / (sc * sc)
            acc = np.zeros((Hh, W, 3), np.float32)
            ws = np.zeros((Hh, W), np.float32)
            if seam_taps is not None:
                seam_taps.begin(W, Hh, s, hit)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx * s, dy * s
                    hq = _shift(hit, ox, oy, False)                  # False outside the image: such a tap is skipped
                    nq, Pq, cq = _shift(n, ox, oy), _shift(P, ox, oy), _shift(c, ox, oy)
                    dnv = n - nq
                    dn = _dot(dnv, dnv)
                    d = _dot(Pq - P, n)
                    dcv = c - cq
                    dc = _dot(dcv, dcv)
                    e = dn * kn + d * d * kx + dc * kc
                    w = (H5[dx + 2] * H5[dy + 2]) * exp_fn(-e)
                    take = hq & (w > f32(0.0))
                    acc = np.where(take[..., None], acc + w[..., None] * cq, acc)
                    ws = np.where(take, ws + w, ws)
                    if seam_taps is not None:
                        seam_taps.tap(dx, dy, take)
            if seam_taps is not None:
                seam_taps.end()
            res = np.where((ws > f32(0.0))[..., None], acc / ws[..., None], c)
            c = np.where(hit[..., None], res, c).astype(np.float32)
        # 3. finish
        out = (c * a).astype(np.float32)
    out = out.reshape(-1, 3)
    return out, (pack_fn(out) if pack else None)

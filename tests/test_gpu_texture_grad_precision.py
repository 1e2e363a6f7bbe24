"""GPU parity of the texture gradient on MAGNIFIED textures under upstream gradients with outliers.

The texel-gradient kernels (k_tex_grad, k_tex_grad_lean) sum a 16x16-pixel block's taps in an LDS patch table whose number format
is scaled by the block's largest |dy|.  Under magnification many pixels of a block add small terms to the same few texels while one
pixel of the block (an outlier: a silhouette pixel after antialias, a texel-fitting loss with a few bad pixels) sets the scale; the
resolution of the table relative to that scale decides whether those sums stay within the single-op bar of tests/conftest.py.  The
other texture tests sample random uv (minified, few shared texels) or constant uv (identical footprints); these scenes do neither.

Bars: tests/conftest.py `grad_tol` and `within`; uv / uv_da / bias gradients only where the reference function is continuous
(`discontinuous_pixels`).  tests/test_texgrad_precision_model.py holds a numpy model of one block's table at these settings."""
import numpy as np
import pytest
import torch
from conftest import ATOL, discontinuous_pixels, grad_tol, within

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _affine_uv(rng, N, H, W, tex_h, tex_w, mag, angle):
    """uv of a smooth affine map: one texel spans `mag` pixels along the footprint's major axis (1.3 mag along the other, with a
    little shear: an isotropic footprint is a singular point of the reference's uv_da gradient), rotated by `angle`, with a random
    sub-texel offset per image.  Returns uv [N,H,W,2] and its exact pixel differentials uv_da [N,H,W,4] (du/dx, du/dy, dv/dx,
    dv/dy), in texels per pixel divided by the texture extent."""
    c, s = np.cos(angle), np.sin(angle)
    J = np.array([[c, -s], [s, c]]) @ np.array([[1.0, 0.15], [0.0, 1.0 / 1.3]]) / mag      # texels per pixel
    y, x = np.mgrid[0:H, 0:W].astype(np.float64) + 0.5
    x, y = x - 0.5 * W, y - 0.5 * H
    uv = np.zeros((N, H, W, 2), np.float64)
    for n in range(N):
        ox, oy = rng.uniform(0.0, 1.0, size=2)
        uv[n, ..., 0] = (J[0, 0] * x + J[0, 1] * y + ox + 0.5 * tex_w) / tex_w
        uv[n, ..., 1] = (J[1, 0] * x + J[1, 1] * y + oy + 0.5 * tex_h) / tex_h
    da = np.empty((N, H, W, 4), np.float64)
    da[..., 0], da[..., 1] = J[0, 0] / tex_w, J[0, 1] / tex_w
    da[..., 2], da[..., 3] = J[1, 0] / tex_h, J[1, 1] / tex_h
    return uv.astype(np.float32), da.astype(np.float32)


def _outlier_dy(rng, N, H, W, C, outlier, where="random", uv=None, tex_hw=None):
    """dy ~ N(0,1) with ONE outlier pixel of magnitude `outlier` per 16x16 block.  where='random': anywhere in the block;
    where='quarter': at the pixel of the block whose bilinear weights are closest to 1/4 each (|g_tex|_inf is then only about
    outlier/4 where no other outlier reaches the texel)."""
    dy = rng.normal(size=(N, H, W, C))
    for n in range(N):
        for by in range(0, H, 16):
            for bx in range(0, W, 16):
                h, w = min(16, H - by), min(16, W - bx)
                if where == "quarter":
                    f = uv[n, by:by + h, bx:bx + w] * np.array([tex_hw[1], tex_hw[0]]) - 0.5
                    f = np.abs(f - np.floor(f) - 0.5).sum(-1)
                    k = int(np.argmin(f))
                else:
                    k = int(rng.integers(h * w))
                dy[n, by + k // w, bx + k % w] = outlier * rng.choice([-1.0, 1.0], size=C)
    return dy.astype(np.float32)


class _NoFootprint:
    """The oracle for a filter without a footprint, as `discontinuous_pixels` reads it: a gradient w.r.t. uv_da of zero."""
    def __init__(self, oracle):
        self.oracle = oracle

    def texture_grad(self, tex, uv, dy, uv_da, **kw):
        g = dict(self.oracle.texture_grad(tex, uv, dy, **kw))
        g["uv_da"] = np.zeros(uv.shape[:3] + (4,), np.float32)
        return g


def _check(dr, oracle, name, tex, uv, uv_da, bias, dy, fm, bm):
    kw = dict(filter_mode=fm, boundary_mode=bm)
    mip = fm == "linear-mipmap-linear"
    t_tex = _t(tex).requires_grad_(True)
    t_uv = _t(uv).requires_grad_(True)
    t_da = _t(uv_da).requires_grad_(True) if mip else None
    t_bias = _t(bias).requires_grad_(True) if mip else None
    out = dr.texture(t_tex, t_uv, t_da, t_bias, **kw)
    out.backward(_t(dy))
    torch.cuda.synchronize()
    oo = oracle.texture(tex, uv, uv_da if mip else None, bias if mip else None, **kw)
    g = oracle.texture_grad(tex, uv, dy, uv_da if mip else None, bias if mip else None, **kw)
    within(name + " value", out.detach().cpu().numpy(), oo, ATOL)
    within(name + " g_tex", t_tex.grad.cpu().numpy(), g["tex"], grad_tol(g["tex"]))
    if mip:
        ok = ~discontinuous_pixels(oracle, tex, uv, dy, uv_da, dict(kw, mip_level_bias=bias))
    else:
        ok = ~discontinuous_pixels(_NoFootprint(oracle), tex, uv, dy, np.zeros(uv.shape[:3] + (4,), np.float32), kw)
    assert ok.mean() > 0.99, ("too many pixels at a discontinuity", 1.0 - ok.mean())
    within(name + " g_uv", t_uv.grad.cpu().numpy(), g["uv"], grad_tol(g["uv"]), where=ok)
    if mip:
        within(name + " g_uv_da", t_da.grad.cpu().numpy(), g["uv_da"], grad_tol(g["uv_da"]), where=ok)
        within(name + " g_bias", t_bias.grad.cpu().numpy(), g["mip_level_bias"], grad_tol(g["mip_level_bias"]), where=ok)
    return g


# (texture size, C, tex_n == N, magnification, filter, boundary, outlier, outlier position): every value of each axis at least
# once; 2 x 192^2 pixels each, 14 scenes: about 1 M pixels in all.  With the table scaled by the block's largest |dy| alone, the
# scenes with an outlier placed at bilinear weights of 1/4 and several others reached 1.86x the bar.
SCENES = [
    (8, 1, False, 4, "linear", "wrap", 10.0, "random"),
    (16, 3, True, 8, "linear", "clamp", 10.0, "random"),
    (16, 3, False, 8, "linear", "wrap", 100.0, "quarter"),
    (32, 4, False, 16, "linear", "wrap", 100.0, "random"),
    (64, 3, True, 32, "linear", "clamp", 10.0, "random"),
    (16, 1, False, 32, "linear", "wrap", 1000.0, "quarter"),
    (32, 3, False, 32, "linear", "wrap", 10.0, "quarter"),
    (8, 4, True, 16, "linear", "clamp", 1000.0, "random"),
    (16, 3, False, 4, "linear-mipmap-linear", "wrap", 100.0, "random"),
    (32, 1, True, 8, "linear-mipmap-linear", "clamp", 10.0, "quarter"),
    (64, 4, False, 16, "linear-mipmap-linear", "wrap", 1000.0, "random"),
    (16, 3, False, 32, "linear-mipmap-linear", "clamp", 100.0, "quarter"),
    (8, 3, False, 32, "linear-mipmap-linear", "wrap", 10.0, "random"),
    (64, 3, True, 8, "linear-mipmap-linear", "wrap", 1000.0, "quarter"),
]


@pytest.mark.parametrize("size,C,per_image,mag,fm,bm,outlier,where", SCENES)
def test_magnified_texture_with_outliers(dr, oracle, size, C, per_image, mag, fm, bm, outlier, where):
    rng = np.random.default_rng(size * 1000 + C * 100 + mag + int(outlier))
    N, H, W = 2, 192, 192
    tex = rng.uniform(size=(N if per_image else 1, size, size, C)).astype(np.float32)
    uv, uv_da = _affine_uv(rng, N, H, W, size, size, mag, angle=rng.uniform(0.05, 0.4))
    # linear-mipmap-linear: the footprint alone selects a level below 0 (clamped to 0); the bias lifts it to between 0 and 1 so that
    # level 1 takes taps too
    bias = (np.log2(mag) + rng.uniform(0.2, 0.8, size=(N, H, W))).astype(np.float32)
    dy = _outlier_dy(rng, N, H, W, C, outlier, where, uv, (size, size))
    _check(dr, oracle, "magnified texture", tex, uv, uv_da, bias, dy, fm, bm)


@pytest.mark.parametrize("fm", ["linear", "linear-mipmap-linear"])
def test_magnified_texture_silhouette_band(dr, oracle, fm):
    """A high-|dy| band one to two pixels wide along a slanted line -- an antialiased silhouette -- over small N(0,1) terms."""
    rng = np.random.default_rng(77)
    N, H, W, C, size, mag = 2, 256, 256, 3, 16, 16
    tex = rng.uniform(size=(1, size, size, C)).astype(np.float32)
    uv, uv_da = _affine_uv(rng, N, H, W, size, size, mag, angle=0.1)
    bias = np.full((N, H, W), np.log2(mag) + 0.5, np.float32)
    dy = rng.normal(size=(N, H, W, C))
    y, x = np.mgrid[0:H, 0:W] + 0.5
    band = np.abs(0.37 * x - y + 90.0) < 1.2
    dy[:, band] *= 300.0
    _check(dr, oracle, "magnified texture band", tex, uv, uv_da, bias, dy.astype(np.float32), fm, "wrap")


def test_magnified_texture_through_the_chain(dr, oracle):
    """rasterize -> interpolate (with pixel differentials) -> texture on a mesh with a 16^2 texture drawn at about 20x, one outlier
    per block; the texture gradient against the oracle on the uv the GPU interpolated (single-op bar)."""
    rng = np.random.default_rng(5)
    res = 320
    n = 6                                                         # a 6x6 grid of quads, uv over the whole texture
    gx, gy = np.meshgrid(np.linspace(-0.95, 0.95, n + 1), np.linspace(-0.95, 0.95, n + 1))
    jit = rng.uniform(-0.03, 0.03, size=gx.shape + (2,))
    pos = np.stack([gx + jit[..., 0], gy + jit[..., 1], 0.1 * np.sin(3 * gx), np.ones_like(gx)], -1).reshape(-1, 4)
    uvv = np.stack([(gx + 1) / 2, (gy + 1) / 2], -1).reshape(-1, 2)
    tri = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            tri += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    pos = _t(np.ascontiguousarray(pos[None].astype(np.float32)))
    tri = _t(np.array(tri, np.int32))
    ctx = dr.RasterizeCudaContext(device="cuda")
    rast, rast_db = dr.rasterize(ctx, pos, tri, (res, res))
    uv, uv_da = dr.interpolate(_t(uvv.astype(np.float32)), rast, tri, rast_db=rast_db, diff_attrs="all")
    uv_np, da_np = uv.cpu().numpy(), uv_da.cpu().numpy()
    C, size = 3, 16
    tex = rng.uniform(size=(1, size, size, C)).astype(np.float32)
    dy = _outlier_dy(rng, 1, res, res, C, 100.0)
    dy[rast[..., 3].cpu().numpy() == 0] = 0.0                        # no gradient on the background
    assert (rast[..., 3] > 0).float().mean() > 0.8
    bias = np.full((1, res, res), 4.5, np.float32)
    for fm in ("linear", "linear-mipmap-linear"):
        _check(dr, oracle, "magnified texture chain", tex, uv_np, da_np, bias, dy, fm, "clamp")

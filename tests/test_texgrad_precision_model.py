"""A numpy model of one 16x16-pixel block of the texture gradient's LDS patch table (k_tex_grad / k_tex_grad_lean, csrc/texture.hip),
on the scenes tests/test_gpu_texture_grad_precision.py runs on the GPU: a magnified texture, dy ~ N(0, 1) with one outlier per block.

Modelled: the block's pixels in the kernels' lane order (8x8-pixel tiles, one per wave; 16-lane DPP rows of two pixel rows), the f32
pre-sum over runs of equal footprints inside a 16-lane row (RunScan), the conversion of every run total to fixed point scaled by the
block's dy (FixedScale32), the integer sums, and the conversion of each texel's sum back to f32.  Compared with the f64 sum
of the same terms under the single-op bar of tests/conftest.py, taken over the block's own gradient (|g_tex|_inf of one block is
no larger than that of an image of such blocks, so the model is the stricter of the two).

The table's 32-bit sums are scaled to a bound of every texel's total over the block (4 x the largest wave's sum of |dy|); they must
stay within half the bar on every block of the seed set.  Scaled to the largest |dy| alone, as the table was before, the same sums
reach 1.74x the bar in this model (and measured 1.86x on the GPU)."""
import numpy as np
import pytest

from conftest import ATOL


def _lanes():
    """(py, px) of the 256 threads of a 16x16 block: four 8x8 tiles (one wave each), row-major inside a tile."""
    order = []
    for w in range(4):
        ty, tx = (w // 2) * 8, (w % 2) * 8
        order += [(ty + i // 8, tx + i % 8) for i in range(64)]
    return order


LANES = _lanes()


def _fixed(fmt, dy):
    """to_fixed / to_float of a block's table (nvdr_device.hpp FixedScale32).  "shipped": scaled to a bound B of every texel's total,
    4 x the largest of the four waves' f32 sums of |dy| (one channel here), s = 29 - e with B < 2^(e+1).  "max-scaled": the format
    the table had before, scaled to the largest |dy| M alone, s = 20 - e with M < 2^(e+1)."""
    if fmt == "shipped":
        waves = [np.float32(np.abs([dy[p] for p in LANES[64 * w:64 * w + 64]], dtype=np.float32).sum(dtype=np.float32)) for w in range(4)]
        e = int(np.frexp(np.float32(4) * max(waves))[1]) - 1
        s = 29 - e
    else:
        e = int(np.frexp(np.float32(np.abs(dy).max()))[1]) - 1
        s = 20 - e
    return (lambda x: int(np.rint(np.float64(x) * 2.0 ** s))), (lambda t: np.float32(np.float64(t) * 2.0 ** -s)), s


def _block(rng, mag, outlier, tex=16):
    """uv (texel units) and dy of one block of an affine magnified map with a random sub-texel offset and angle."""
    a = rng.uniform(0.05, 0.4)
    c, s = np.cos(a), np.sin(a)
    J = np.array([[c, -s], [s, c]]) @ np.array([[1.0, 0.15], [0.0, 1.0 / 1.3]]) / mag
    o = rng.uniform(0, tex, size=2)
    py, px = np.mgrid[0:16, 0:16].astype(np.float64) + 0.5
    u = (J[0, 0] * px + J[0, 1] * py + o[0]) / tex
    v = (J[1, 0] * px + J[1, 1] * py + o[1]) / tex
    uv = np.stack([u, v], -1).astype(np.float32)
    dy = rng.normal(size=(16, 16)).astype(np.float32)
    k = rng.integers(256)
    dy[k // 16, k % 16] = outlier * rng.choice([-1.0, 1.0])
    return uv, dy


def _taps(uv, tex):
    """Texel indices and bilinear weights of each pixel, in f32 as the kernels compute them, and in f64 as the oracle does."""
    x = uv[..., 0].astype(np.float32) * np.float32(tex) - np.float32(0.5)
    y = uv[..., 1].astype(np.float32) * np.float32(tex) - np.float32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fu, fv = (x - x0).astype(np.float32), (y - y0).astype(np.float32)
    w11 = fu * fv
    w10, w01 = fu - w11, fv - w11
    w00 = np.float32(1) - fu - w01
    w32 = np.stack([w00, w10, w01, w11], -1).astype(np.float32)
    f64u, f64v = fu.astype(np.float64), fv.astype(np.float64)
    w64 = np.stack([(1 - f64u) * (1 - f64v), f64u * (1 - f64v), (1 - f64u) * f64v, f64u * f64v], -1)
    xi, yi = x0.astype(np.int64), y0.astype(np.int64)
    idx = np.stack([(yi % tex) * tex + xi % tex, (yi % tex) * tex + (xi + 1) % tex,
                    ((yi + 1) % tex) * tex + xi % tex, ((yi + 1) % tex) * tex + (xi + 1) % tex], -1)
    return idx, w32, w64, np.stack([xi, yi], -1)


def block_error(fmt, uv, dy, tex=16):
    """Worst |table result - f64 sum| over the block's texels, as a fraction of the single-op bar of the block's gradient."""
    idx, w32, w64, quad = _taps(uv, tex)
    exact = np.zeros(tex * tex)
    np.add.at(exact, idx.reshape(-1), (w64 * dy.astype(np.float64)[..., None]).reshape(-1))
    to_fixed, to_float, s = _fixed(fmt, dy)
    acc = {}
    run = np.zeros(4, np.float32)
    for lane, (py, px) in enumerate(LANES):
        term = (w32[py, px] * dy[py, px]).astype(np.float32)
        same = lane % 16 != 0 and (quad[py, px] == quad[LANES[lane - 1]]).all()
        run = (run + term).astype(np.float32) if same else term
        nxt = LANES[lane + 1] if lane + 1 < 256 else None
        tail = nxt is None or (lane + 1) % 16 == 0 or not (quad[nxt] == quad[py, px]).all()
        if tail:
            for k in range(4):
                t = int(idx[py, px, k])
                acc[t] = acc.get(t, 0) + to_fixed(run[k])
    got = np.zeros(tex * tex)
    for t, v in acc.items():
        assert abs(v) < 2 ** 31 - 1, (fmt, t, v)                       # the int32 cell never overflows
        got[t] = to_float(v)
    return float(np.abs(got - exact).max()) / (ATOL * max(1.0, float(np.abs(exact).max())))


SCENES = [(8, 10.0), (16, 100.0), (32, 10.0)]       # (magnification, outlier)


def _errors(fmt, mag, outlier, blocks=120, seed=0):
    rng = np.random.default_rng(seed * 1000 + mag)
    return np.array([block_error(fmt, *_block(rng, mag, outlier)) for _ in range(blocks)])


@pytest.mark.parametrize("mag,outlier", SCENES)
def test_shipped_patch_table_format_stays_within_half_the_bar(mag, outlier):
    e = _errors("shipped", mag, outlier)
    assert e.max() <= 0.5, (mag, outlier, e.max())


def test_shipped_format_without_outliers_and_at_full_scale():
    """Blocks of N(0, 1) alone (no outlier) at 32x, and blocks whose every |dy| is the same large value (the bound at its largest,
    256 M: the coarsest resolution the format takes, 2^-22 M) -- within half the bar, and no cell near 2^31."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(60):
        uv, dy = _block(rng, 32, 1.0)
        worst = max(worst, block_error("shipped", uv, dy))
        worst = max(worst, block_error("shipped", uv, np.float32(1.99e4) * np.sign(dy).astype(np.float32)))
    assert worst <= 0.5, worst


def test_the_model_sees_the_max_scaled_failure():
    """The model is worth its assertions only if it reproduces what the GPU measured with the table scaled by the largest |dy|
    (1.86x the bar on tests/test_gpu_texture_grad_precision.py's scenes): blocks beyond the bar."""
    worst = max(_errors("max-scaled", mag, outlier).max() for mag, outlier in SCENES)
    assert worst > 1.0, worst

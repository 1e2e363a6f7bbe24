"""GPU parity on both sides of every switch of the gradient kernels' reduction strategy.

The host side of texture_grad, interpolate_grad and interpolate_rasterize_grad sizes an LDS table from the channel / attribute count
(csrc/nvdr_plan.hpp), drops it beyond the texture key format, spills taps the full table cannot place, and picks scalar instead of
vector kernels for misaligned pointers or extents.  Each test below runs a shape on one side of one switch; PLAN_CLAIMS states which
side, and tests/test_reduction_plan.py checks the claims against nvdr_plan.hpp itself, so a retuned threshold cannot leave a pair
of tests on the same side unnoticed.

Bars: tests/conftest.py (`grad_tol`, `within`, `discontinuous_pixels`)."""
import numpy as np
import pytest
import torch
from conftest import ATOL, discontinuous_pixels, grad_tol, within

from nvdiffrast_amd.utils import m10k_batch

pytestmark = pytest.mark.gpu

TEX_C = [6, 7, 12, 13, 25, 26, 32]
INTERP_A = [4, 5, 9, 10, 19, 20, 39, 40, 79, 80, 255, 256, 300]
FUSED_A = [4, 5, 252, 253, 300]
IP_BLOCK = (64, 16)                 # k_interp_grad's and k_interp_raster_grad's pixel block (interpolate.hip, backward_fused.hip)
TEX_BLOCK = 16                      # k_tex_grad's 16x16-pixel block

# Which side of each switch the tests run: (plan function of nvdr_plan.hpp, its arguments, the value it must return, the tests).
# tex_grad_groups(C, tex_w, tex_h, cube): patches of the texture-gradient table (0: no table).  interp_grad_slots(A) and
# fused_grad_slots(A): vertex-table slots (0: no table).
PLAN_CLAIMS = [
    ("tex_grad_groups", (6, 64, 32, 0), 64, "test_texture_channel_count[6-*]"),
    ("tex_grad_groups", (7, 64, 32, 0), 32, "test_texture_channel_count[7-*]"),
    ("tex_grad_groups", (12, 64, 32, 0), 32, "test_texture_channel_count[12-*]"),
    ("tex_grad_groups", (13, 64, 32, 0), 16, "test_texture_channel_count[13-*]"),
    ("tex_grad_groups", (25, 64, 32, 0), 16, "test_texture_channel_count[25-*]"),
    ("tex_grad_groups", (26, 64, 32, 0), 0, "test_texture_channel_count[26-*]"),
    ("tex_grad_groups", (32, 64, 32, 0), 0, "test_texture_channel_count[32-*]"),
    ("tex_grad_groups", (26, 16, 16, 1), 0, "test_cube_texture_without_a_table"),
    ("tex_grad_groups", (3, 256, 256, 0), 128, "test_texture_table_overflow[3-*]"),
    ("tex_grad_groups", (13, 256, 256, 0), 16, "test_texture_table_overflow[13-*]"),
    ("tex_grad_groups", (25, 256, 256, 0), 16, "test_texture_table_overflow[25-*]"),
    ("tex_grad_groups", (3, 32768, 2, 0), 128, "test_texture_key_limit[width-32768]"),
    ("tex_grad_groups", (3, 32769, 2, 0), 0, "test_texture_key_limit[width-32769]"),
    ("tex_grad_groups", (1, 1, 65536, 0), 256, "test_texture_key_limit[height-65536]"),
    ("interp_grad_slots", (4,), 512, "test_interpolate_grad_table_sizes[4-*]"),
    ("interp_grad_slots", (5,), 256, "test_interpolate_grad_table_sizes[5-*]"),
    ("interp_grad_slots", (9,), 256, "test_interpolate_grad_table_sizes[9-*]"),
    ("interp_grad_slots", (10,), 128, "test_interpolate_grad_table_sizes[10-*]"),
    ("interp_grad_slots", (19,), 128, "test_interpolate_grad_table_sizes[19-*]"),
    ("interp_grad_slots", (20,), 64, "test_interpolate_grad_table_sizes[20-*]"),
    ("interp_grad_slots", (39,), 64, "test_interpolate_grad_table_sizes[39-*]"),
    ("interp_grad_slots", (40,), 32, "test_interpolate_grad_table_sizes[40-*]"),
    ("interp_grad_slots", (79,), 32, "test_interpolate_grad_table_sizes[79-*]"),
    ("interp_grad_slots", (80,), 32, "test_interpolate_grad_table_sizes[80-*] (above 20 KiB)"),
    ("interp_grad_slots", (255,), 32, "test_interpolate_grad_table_sizes[255-*]"),
    ("interp_grad_slots", (256,), 0, "test_interpolate_grad_table_sizes[256-*]"),
    ("interp_grad_slots", (300,), 0, "test_interpolate_grad_table_sizes[300-*]"),
    ("fused_grad_slots", (4,), 512, "test_fused_grad_table_sizes[4-*]"),
    ("fused_grad_slots", (5,), 256, "test_fused_grad_table_sizes[5-*]"),
    ("fused_grad_slots", (252,), 32, "test_fused_grad_table_sizes[252-*]"),
    ("fused_grad_slots", (253,), 0, "test_fused_grad_table_sizes[253-*]"),
    ("fused_grad_slots", (300,), 0, "test_fused_grad_table_sizes[300-*]"),
    ("interp_grad_slots", (4,), 512, "test_vertex_table_overflow[4]"),
    ("interp_grad_slots", (40,), 32, "test_vertex_table_overflow[40]"),
    ("fused_grad_slots", (4,), 512, "test_vertex_table_overflow[4]"),
    ("fused_grad_slots", (40,), 64, "test_vertex_table_overflow[40]"),
]
# the table size against which test_vertex_table_overflow must see more distinct vertices in one pixel block
OVERFLOW_SLOTS = {4: 512, 40: 64}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _misaligned(a):
    """A contiguous CUDA tensor equal to `a` whose data starts one float past an aligned address (storage_offset 1)."""
    a = np.ascontiguousarray(a, np.float32)
    base = torch.empty(a.size + 1, device="cuda")
    v = base[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 8 == 4
    return v


# ------------------------------------------------------------------------------------------------------------------- texture

def _texture_check(dr, oracle, name, tex, uv, uv_da, bias, dy, fm, bm, max_mip_level=None, min_ok=0.98):
    kw = dict(filter_mode=fm, boundary_mode=bm)
    if max_mip_level is not None:
        kw["max_mip_level"] = max_mip_level
    mip = fm == "linear-mipmap-linear"
    t_tex = _t(tex).requires_grad_(True)
    t_uv = _t(uv).requires_grad_(True)
    t_da = _t(uv_da).requires_grad_(True) if (mip and uv_da is not None) else None
    t_bias = _t(bias).requires_grad_(True) if (mip and bias is not None) else None
    out = dr.texture(t_tex, t_uv, t_da, t_bias, **kw)
    out.backward(_t(dy))
    torch.cuda.synchronize()
    da = uv_da if mip else None
    b = bias if mip else None
    within(name + " value", out.detach().cpu().numpy(), oracle.texture(tex, uv, da, b, **kw), ATOL)
    g = oracle.texture_grad(tex, uv, dy, da, b, **kw)
    within(name + " g_tex", t_tex.grad.cpu().numpy(), g["tex"], grad_tol(g["tex"]))
    ok = None
    if mip and uv_da is not None:
        ok = ~discontinuous_pixels(oracle, tex, uv, dy, uv_da, dict(kw, mip_level_bias=bias))
        assert ok.mean() >= min_ok and ok.any(), 1.0 - ok.mean()
        within(name + " g_uv_da", t_da.grad.cpu().numpy(), g["uv_da"], grad_tol(g["uv_da"]), where=ok)
    if t_bias is not None:
        within(name + " g_bias", t_bias.grad.cpu().numpy(), g["mip_level_bias"], grad_tol(g["mip_level_bias"]), where=ok)
    if uv.shape[-1] == 2 and not mip:
        class _NoFootprint:
            def texture_grad(self, tex, uv, dy, uv_da, **k):
                r = dict(oracle.texture_grad(tex, uv, dy, **k))
                r["uv_da"] = np.zeros(uv.shape[:3] + (4,), np.float32)
                return r
        ok = ~discontinuous_pixels(_NoFootprint(), tex, uv, dy, np.zeros(uv.shape[:3] + (4,), np.float32), kw)
        assert ok.mean() >= min_ok and ok.any(), 1.0 - ok.mean()
    within(name + " g_uv", t_uv.grad.cpu().numpy(), g["uv"], grad_tol(g["uv"]), where=ok)


def _smooth_uv(rng, N, H, W, tex_h, tex_w, texels_per_pixel):
    """uv of an anisotropic affine map (texels_per_pixel along x, 0.8 of it along y, slight shear) and its pixel differentials."""
    J = np.array([[1.0, 0.2], [-0.15, 0.8]]) * texels_per_pixel
    y, x = np.mgrid[0:H, 0:W].astype(np.float64) + 0.5
    uv = np.zeros((N, H, W, 2))
    for n in range(N):
        o = rng.uniform(0, 1, size=2) * [tex_w, tex_h]
        uv[n, ..., 0] = (J[0, 0] * x + J[0, 1] * y + o[0]) / tex_w
        uv[n, ..., 1] = (J[1, 0] * x + J[1, 1] * y + o[1]) / tex_h
    da = np.empty((N, H, W, 4))
    da[..., 0], da[..., 1] = J[0, 0] / tex_w, J[0, 1] / tex_w
    da[..., 2], da[..., 3] = J[1, 0] / tex_h, J[1, 1] / tex_h
    return uv.astype(np.float32), da.astype(np.float32)


@pytest.mark.parametrize("bm", ["wrap", "clamp"])
@pytest.mark.parametrize("fm", ["linear", "linear-mipmap-linear"])
@pytest.mark.parametrize("C", TEX_C)
def test_texture_channel_count(dr, oracle, C, fm, bm):
    """Texture C on both sides of the patch table's 64 -> 32 -> 16 -> none steps (the general kernel: C > 4)."""
    rng = np.random.default_rng(C * 10 + len(fm) + len(bm))
    N, H, W, th, tw = 2, 40, 48, 32, 64
    tex = rng.uniform(size=(1, th, tw, C)).astype(np.float32)
    uv, uv_da = _smooth_uv(rng, N, H, W, th, tw, 0.7)
    bias = rng.uniform(0.3, 1.7, size=(N, H, W)).astype(np.float32)
    dy = rng.normal(size=(N, H, W, C)).astype(np.float32)
    dy[0, :5] = 0.0
    _texture_check(dr, oracle, "texture C=%d" % C, tex, uv, uv_da, bias, dy, fm, bm)


def test_cube_texture_without_a_table(dr, oracle):
    rng = np.random.default_rng(26)
    N, H, W, C = 2, 24, 20, 26
    tex = rng.uniform(size=(1, 6, 16, 16, C)).astype(np.float32)
    v = rng.normal(size=(N, H, W, 3)).astype(np.float32)
    da = (rng.normal(size=(N, H, W, 6)) * 0.2).astype(np.float32)
    dy = rng.normal(size=(N, H, W, C)).astype(np.float32)
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode="cube")
    t_tex = _t(tex).requires_grad_(True)
    t_v = _t(v).requires_grad_(True)
    t_da = _t(da).requires_grad_(True)
    out = dr.texture(t_tex, t_v, t_da, **kw)
    out.backward(_t(dy))
    within("cube C=26 value", out.detach().cpu().numpy(), oracle.texture(tex, v, da, **kw), ATOL)
    g = oracle.texture_grad(tex, v, dy, da, **kw)
    within("cube C=26 g_tex", t_tex.grad.cpu().numpy(), g["tex"], grad_tol(g["tex"]))
    within("cube C=26 g_uv", t_v.grad.cpu().numpy(), g["uv"], grad_tol(g["uv"]))
    within("cube C=26 g_uv_da", t_da.grad.cpu().numpy(), g["uv_da"], grad_tol(g["uv_da"]))


@pytest.mark.parametrize("fm", ["linear", "linear-mipmap-linear"])
@pytest.mark.parametrize("C", [3, 13, 25])
def test_texture_table_overflow(dr, oracle, C, fm):
    """Random uv over a 256^2 texture: every 16x16-pixel block taps far more 8x2-texel patches than the table holds, so
    most taps find no slot within 8 probes and go to memory (asserted on the host from the tap positions)."""
    rng = np.random.default_rng(C)
    N, H, W, ts = 1, 48, 64, 256
    tex = rng.uniform(size=(1, ts, ts, C)).astype(np.float32)
    uv = rng.uniform(0.0, 1.0, size=(N, H, W, 2)).astype(np.float32)
    uv_da = (rng.normal(size=(N, H, W, 4)) * 0.004).astype(np.float32)
    dy = rng.normal(size=(N, H, W, C)).astype(np.float32)
    x0 = np.floor(uv[..., 0] * ts - 0.5).astype(np.int64)
    y0 = np.floor(uv[..., 1] * ts - 0.5).astype(np.int64)
    worst = 0
    for by in range(0, H, TEX_BLOCK):
        for bx in range(0, W, TEX_BLOCK):
            xs, ys = x0[0, by:by + 16, bx:bx + 16], y0[0, by:by + 16, bx:bx + 16]
            keys = {((x + dx) % ts >> 3, (y + dy_) % ts >> 1) for x, y in zip(xs.ravel(), ys.ravel()) for dx in (0, 1) for dy_ in (0, 1)}
            worst = max(worst, len(keys))
    assert worst > 2 * 128, worst                               # far beyond the 16 (C = 13, 25) or 128 (C = 3) patches of the table
    # (random minified uv: a one-ulp nudge of uv moves a tap by 256 ulp of a texel, so more pixels than in a smooth scene are within
    #  rounding distance of a texel or level boundary by the named criterion; g_tex, what this test is about, is compared everywhere)
    _texture_check(dr, oracle, "texture table overflow", tex, uv, uv_da, None, dy, fm, "wrap", min_ok=0.8)


@pytest.mark.parametrize("axis,extent", [("width", 32768), ("width", 32769), ("height", 65536), ("height", 65537)])
def test_texture_key_limit(dr, oracle, axis, extent):
    """Textures at the patch key's limit (x < 32768 texels in patch columns of 8, y < 65536): uv near the far edge so that taps land
    on the last texels and wrap to texel 0, magnified so that the taps share patches.  A 2-D texture taller than 65536 texels is
    refused with the reference's message (torch_texture.cpp: at most 2^16 texels per side), so the key format's height limit is
    reached only by cube maps of more than 10922 texels per face, which no test here runs (PLAN_CLAIMS makes no claim for it)."""
    rng = np.random.default_rng(extent)
    C = 3 if axis == "width" else 1
    shape = (1, 2, extent, C) if axis == "width" else (1, extent, 1, C)
    tex = rng.uniform(size=shape).astype(np.float32)
    if axis == "height" and extent > 65536:
        with pytest.raises(RuntimeError, match="texture size too large"):
            dr.texture(_t(tex), torch.full((1, 4, 4, 2), 0.5, device="cuda"), filter_mode="linear")
        return
    N, H, W = 1, 16, 64
    y, x = np.mgrid[0:H, 0:W].astype(np.float64) + 0.5
    far = (extent - 8 + x * 0.25) / extent                     # texels extent-8 .. extent+8: the last ones, then wrapped to 0..
    uv = np.zeros((N, H, W, 2))
    if axis == "width":
        uv[0, ..., 0], uv[0, ..., 1] = far, (y * 0.13) / 2
    else:
        uv[0, ..., 0], uv[0, ..., 1] = 0.3, far
    uv = uv.astype(np.float32)
    dy = rng.normal(size=(N, H, W, C)).astype(np.float32)
    # (at 2^15..2^16 texels per unit uv one ulp of uv is 1/256 of a texel or more: the uv gradient of most pixels moves by more than
    #  its bar under the named criterion's nudge and is excluded by it; g_tex -- the table -- is compared everywhere)
    _texture_check(dr, oracle, "texture key limit", tex, uv, None, None, dy, "linear", "wrap", min_ok=0.0)
    _texture_check(dr, oracle, "texture key limit", tex, uv, None, None, dy, "linear", "clamp", min_ok=0.0)


@pytest.mark.parametrize("tex_w", [18, 20])
def test_mip_gradient_pass_scalar_and_vector(dr, oracle, tex_w):
    """Texture width 18 (not a multiple of 4: the scalar k_mip_grad) against 20 (k_mip_grad_vec)."""
    rng = np.random.default_rng(tex_w)
    N, H, W, C = 2, 24, 24, 3
    tex = rng.uniform(size=(1, 16, tex_w, C)).astype(np.float32)
    uv, uv_da = _smooth_uv(rng, N, H, W, 16, tex_w, 1.1)
    bias = rng.uniform(0.1, 0.9, size=(N, H, W)).astype(np.float32)
    dy = rng.normal(size=(N, H, W, C)).astype(np.float32)
    _texture_check(dr, oracle, "mip grad w=%d" % tex_w, tex, uv, uv_da, bias, dy, "linear-mipmap-linear", "wrap", max_mip_level=1)


# --------------------------------------------------------------------------------------------------------------- interpolate

def _interp_scene(N=2, res=(48, 80), seed=3):
    import oracle as raw
    b = m10k_batch(N, seed=seed, nx=20, ny=10)
    ro, rdb = raw.rasterize(b["pos"], b["tri"], res)
    return b, ro, rdb


def _diff_list(A):
    return [int(i) for i in np.unique(np.linspace(0, A - 1, min(A, 32)).astype(int))][::-1]


@pytest.mark.parametrize("attr_mode", ["broadcast", "instance"])
@pytest.mark.parametrize("db", ["none", "all", "list"])
@pytest.mark.parametrize("A", INTERP_A)
def test_interpolate_grad_table_sizes(dr, oracle, A, db, attr_mode):
    b, ro, rdb = _interp_scene()
    N, H, W = ro.shape[:3]
    V = b["pos"].shape[1]
    rng = np.random.default_rng(A)
    # (small attributes: the scene's rast_db reaches a few hundred, and the interpolated differentials must stay where the forward
    #  bar of 1e-5 abs is above their f32 ulp)
    attr = rng.uniform(-0.05, 0.05, size=(1 if attr_mode == "broadcast" else N, V, A)).astype(np.float32)
    dy = rng.normal(size=(N, H, W, A)).astype(np.float32)
    diff = None if db == "none" else ("all" if db == "all" else _diff_list(A))
    D = 0 if diff is None else (A if diff == "all" else len(diff))
    t_attr = _t(attr).requires_grad_(True)
    t_rast = _t(ro).requires_grad_(True)
    t_db = _t(rdb).requires_grad_(True) if diff is not None else None
    out, da = dr.interpolate(t_attr, t_rast, _t(b["tri"]), rast_db=t_db, diff_attrs=diff)
    oo, oda = oracle.interpolate(attr, ro, b["tri"], rast_db=rdb if diff is not None else None, diff_attrs=diff)
    within("interp A=%d value" % A, out.detach().cpu().numpy(), oo, ATOL)
    if diff is None:
        out.backward(_t(dy))
        ga, gr, _ = oracle.interpolate_grad(attr, ro, b["tri"], dy)
    else:
        within("interp A=%d da" % A, da.detach().cpu().numpy(), oda, ATOL)
        dda = rng.normal(size=(N, H, W, 2 * D)).astype(np.float32)
        torch.autograd.backward([out, da], [_t(dy), _t(dda)])
        ga, gr, gdb = oracle.interpolate_grad(attr, ro, b["tri"], dy, rast_db=rdb, dda=dda, diff_attrs=diff)
        within("interp A=%d g_rast_db" % A, t_db.grad.cpu().numpy(), gdb, grad_tol(gdb))
    within("interp A=%d g_attr" % A, t_attr.grad.cpu().numpy(), ga, grad_tol(ga))
    within("interp A=%d g_rast" % A, t_rast.grad.cpu().numpy(), gr, grad_tol(gr))


@pytest.mark.usefixtures("python_host_layer")
@pytest.mark.parametrize("with_da", [False, True])
@pytest.mark.parametrize("with_g_rast", [True, False])
@pytest.mark.parametrize("A", FUSED_A)
def test_fused_grad_table_sizes(dr, oracle, A, with_g_rast, with_da):
    """The fused kernel through _plugin.interpolate_rasterize_grad (as tests/test_gpu_fused_backward.py calls it), against the oracle
    and the two separate kernels, on both sides of its 512 -> 256 and 32 -> no table steps."""
    from nvdiffrast_amd.torch import _plugin
    b, ro, rdb = _interp_scene(seed=4)
    N, H, W = ro.shape[:3]
    V = b["pos"].shape[1]
    rng = np.random.default_rng(A + 1)
    attr = rng.uniform(-1, 1, size=(N, V, A)).astype(np.float32)
    dy = rng.normal(size=(N, H, W, A)).astype(np.float32)
    kw = {}
    dda = None
    if with_da:
        dda = rng.normal(size=(N, H, W, 2 * A)).astype(np.float32)
        kw = dict(rast_db=_t(rdb), dda=_t(dda), diff_attrs_all=True)
        ga, gr, gdb = oracle.interpolate_grad(attr, ro, b["tri"], dy, rast_db=rdb, dda=dda, diff_attrs="all")
    else:
        ga, gr, _ = oracle.interpolate_grad(attr, ro, b["tri"], dy)
        gdb = None
    gp = oracle.rasterize_grad(b["pos"], b["tri"], ro, gr, gdb)
    g_attr, g_rast, g_db, g_pos = _plugin.interpolate_rasterize_grad(_t(attr), _t(ro), _t(b["tri"]), _t(b["pos"]), _t(dy),
                                                                    with_g_rast=with_g_rast, **kw)
    name = "fused A=%d" % A
    within(name + " g_attr", g_attr.cpu().numpy(), ga, grad_tol(ga))
    within(name + " g_pos", g_pos.cpu().numpy(), gp, grad_tol(gp))
    if with_g_rast:
        within(name + " g_rast", g_rast.cpu().numpy(), gr, grad_tol(gr))
        if with_da:
            within(name + " g_rast_db", g_db.cpu().numpy(), gdb, grad_tol(gdb))
    else:
        assert g_rast is None
    # the two separate kernels of the same library
    if with_da:
        s_attr, s_rast, s_db = _plugin.interpolate_grad_da(_t(attr), _t(ro), _t(b["tri"]), _t(dy), _t(rdb), _t(dda), True, [])
    else:
        (s_attr, s_rast), s_db = _plugin.interpolate_grad(_t(attr), _t(ro), _t(b["tri"]), _t(dy)), None
    s_pos = _plugin.rasterize_grad_db(_t(b["pos"]), _t(b["tri"]), _t(ro), s_rast, s_db) if with_da else \
        _plugin.rasterize_grad(_t(b["pos"]), _t(b["tri"]), _t(ro), s_rast)
    within(name + " vs separate g_attr", g_attr.cpu().numpy(), s_attr.cpu().numpy(), grad_tol(ga))
    within(name + " vs separate g_pos", g_pos.cpu().numpy(), s_pos.cpu().numpy(), grad_tol(gp))


def _dense_mesh(n, jitter, seed):
    """An n x n grid of quads over the viewport, vertices jittered: more triangles than pixels at a small resolution."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-0.98, 0.98, n + 1)
    gx, gy = np.meshgrid(g, g)
    d = (g[1] - g[0]) * jitter
    pos = np.stack([gx + rng.uniform(-d, d, gx.shape), gy + rng.uniform(-d, d, gx.shape),
                    rng.uniform(-0.5, 0.5, gx.shape), np.ones_like(gx)], -1).reshape(1, -1, 4).astype(np.float32)
    i = np.arange(n)[None, :] + (n + 1) * np.arange(n)[:, None]
    a, bb, c, dd = i.ravel(), i.ravel() + 1, i.ravel() + n + 2, i.ravel() + n + 1
    tri = np.concatenate([np.stack([a, bb, c], 1), np.stack([a, c, dd], 1)]).astype(np.int32)
    return pos, tri


@pytest.mark.usefixtures("python_host_layer")
@pytest.mark.parametrize("A", [4, 40])
def test_vertex_table_overflow(dr, oracle, A):
    """256 x 256 jittered quads at 128^2: every 64x16 pixel block touches more vertices than the vertex table can place, so part of
    a triangle's vertices go to memory (interpolate grad and the fused kernel's partly tabled triangles)."""
    from nvdiffrast_amd.torch import _plugin
    pos, tri = _dense_mesh(256, 0.3, seed=A)
    res = (128, 128)
    ro, rdb = oracle.rasterize(pos, tri, res)
    ids = ro[0, ..., 3].astype(np.int64)
    worst = 0
    for by in range(0, res[0], IP_BLOCK[1]):
        for bx in range(0, res[1], IP_BLOCK[0]):
            t = ids[by:by + IP_BLOCK[1], bx:bx + IP_BLOCK[0]]
            t = np.unique(t[t > 0]) - 1
            worst = max(worst, np.unique(tri[t]).size)
    assert worst > OVERFLOW_SLOTS[A] + 8, (worst, OVERFLOW_SLOTS[A])       # more distinct vertices than slots (+ 8 probes)
    rng = np.random.default_rng(A)
    V = pos.shape[1]
    attr = rng.uniform(-1, 1, size=(1, V, A)).astype(np.float32)
    dy = rng.normal(size=(1,) + res + (A,)).astype(np.float32)
    ga, gr, _ = oracle.interpolate_grad(attr, ro, tri, dy)
    gp = oracle.rasterize_grad(pos, tri, ro, gr)
    s_attr, s_rast = _plugin.interpolate_grad(_t(attr), _t(ro), _t(tri), _t(dy))
    within("overflow interp A=%d g_attr" % A, s_attr.cpu().numpy(), ga, grad_tol(ga))
    within("overflow interp A=%d g_rast" % A, s_rast.cpu().numpy(), gr, grad_tol(gr))
    g_attr, g_rast, _, g_pos = _plugin.interpolate_rasterize_grad(_t(attr), _t(ro), _t(tri), _t(pos[0]), _t(dy))
    within("overflow fused A=%d g_attr" % A, g_attr.cpu().numpy(), ga, grad_tol(ga))
    within("overflow fused A=%d g_pos" % A, g_pos.cpu().numpy(), gp, grad_tol(gp))
    within("overflow fused A=%d g_rast" % A, g_rast.cpu().numpy(), gr, grad_tol(gr))


# ------------------------------------------------------------------------------------------------ misaligned contiguous views

@pytest.mark.parametrize("A", [2, 4])
def test_misaligned_attr_and_dy(dr, oracle, A):
    """attr / dy one float past an aligned address: the scalar paths of k_interp_fwd, k_interp_grad and the fused kernel instead of
    their float2 / float4 paths.  The reference accepts such tensors (no alignment check on attr or dy)."""
    from nvdiffrast_amd.torch import _plugin
    b, ro, rdb = _interp_scene(seed=5)
    N, H, W = ro.shape[:3]
    V = b["pos"].shape[1]
    rng = np.random.default_rng(A + 7)
    attr = rng.uniform(-1, 1, size=(N, V, A)).astype(np.float32)
    dy = rng.normal(size=(N, H, W, A)).astype(np.float32)
    oo, _ = oracle.interpolate(attr, ro, b["tri"])
    ga, gr, _ = oracle.interpolate_grad(attr, ro, b["tri"], dy)
    gp = oracle.rasterize_grad(b["pos"], b["tri"], ro, gr)
    # through the operator: misaligned attr (the upstream gradient autograd hands in is its own, aligned tensor)
    t_attr = _misaligned(attr).requires_grad_(True)
    out, _ = dr.interpolate(t_attr, _t(ro), _t(b["tri"]))
    within("misaligned attr value", out.detach().cpu().numpy(), oo, ATOL)
    out.backward(_t(dy))
    within("misaligned attr g_attr", t_attr.grad.cpu().numpy(), ga, grad_tol(ga))
    # directly: misaligned attr and dy
    s_attr, s_rast = _plugin.interpolate_grad(_misaligned(attr), _t(ro), _t(b["tri"]), _misaligned(dy))
    within("misaligned attr+dy g_attr", s_attr.cpu().numpy(), ga, grad_tol(ga))
    within("misaligned attr+dy g_rast", s_rast.cpu().numpy(), gr, grad_tol(gr))
    g_attr, g_rast, _, g_pos = _plugin.interpolate_rasterize_grad(_misaligned(attr), _t(ro), _t(b["tri"]), _t(b["pos"]), _misaligned(dy))
    within("misaligned fused g_attr", g_attr.cpu().numpy(), ga, grad_tol(ga))
    within("misaligned fused g_pos", g_pos.cpu().numpy(), gp, grad_tol(gp))
    within("misaligned fused g_rast", g_rast.cpu().numpy(), gr, grad_tol(gr))


def test_misaligned_antialias_color(dr, oracle):
    """color at C = 4, W = 64 one float past an aligned address: the antialias copy's scalar path."""
    b = m10k_batch(2, seed=8, nx=16, ny=8)
    res = (48, 64)
    ro, _ = oracle.rasterize(b["pos"], b["tri"], res)
    rng = np.random.default_rng(4)
    color = rng.uniform(size=(2,) + res + (4,)).astype(np.float32)
    dy = rng.normal(size=color.shape).astype(np.float32)
    t_col = _misaligned(color).requires_grad_(True)
    t_pos = _t(b["pos"]).requires_grad_(True)
    out = dr.antialias(t_col, _t(ro), t_pos, _t(b["tri"]))
    out.backward(_t(dy))
    oo = oracle.antialias(color, ro, b["pos"], b["tri"])
    gc, gp = oracle.antialias_grad(color, ro, b["pos"], b["tri"], dy)
    assert (oo != color).any(-1).sum() > 50
    within("misaligned antialias value", out.detach().cpu().numpy(), oo, ATOL)
    within("misaligned antialias g_color", t_col.grad.cpu().numpy(), gc, grad_tol(gc))
    within("misaligned antialias g_pos", t_pos.grad.cpu().numpy(), gp, grad_tol(gp))


def test_misaligned_texture_inputs(dr, oracle):
    """The reference checks uv's alignment (torch_texture.cpp:317-337): a misaligned uv must either sample what the oracle samples or
    be refused with the reference's message."""
    rng = np.random.default_rng(9)
    tex = rng.uniform(size=(1, 32, 32, 3)).astype(np.float32)
    uv = rng.uniform(size=(1, 16, 16, 2)).astype(np.float32)
    try:
        out = dr.texture(_t(tex), _misaligned(uv), filter_mode="linear")
    except RuntimeError as e:
        assert "uv input tensor not aligned to float2" in str(e), str(e)
    else:
        within("misaligned uv value", out.cpu().numpy(), oracle.texture(tex, uv, filter_mode="linear"), ATOL)

"""The MBConv block's entry points (csrc/batchnorm.hip, depthwise.hip, se.hip, pool.hip) through
the C-ABI at the smallest shapes at which their host dispatch can go wrong: every (dtype, act,
variant) arm the module-level tests do not reach gets a case here.

Arms reached before this file (package callers + tests): ewvit_bn_fwd / ewvit_bn_bwd for both
dtypes, act 0/1/2, groups 1-3 with accumulate 0 (test_gpu_bn); ewvit_bn_fwd_partials,
ewvit_bn_coef, ewvit_bn_bwd_partials (plain and row_scale), ewvit_bn_bwd_scaled,
ewvit_bn_fwd_drop_add with partials, ewvit_bn_bwd_se, ewvit_bn_se_bwd(_dx),
ewvit_bn_act_se_squeeze, the depthwise row kernels and fused backwards, ewvit_se_forward /
_squeeze_mlp_fwd / _squeeze_mlp_bwd / _gate_excite / _scale, ewvit_scale_add(_drop) and the max
pool in bf16 only (the model runs under bf16 autocast; test_gpu_bn_link, test_gpu_bn_fold,
test_gpu_se, test_gpu_modules, test_gpu_kernels).  Not reached: ewvit_bn_bwd accumulate 1;
ewvit_bn_bwd_reduce in f32 and for act 0 / 2; the f32 arms of _bwd_scaled, _bwd_partials
(row_scale), _bwd_se, _fwd_partials and _fwd_drop_add; _fwd_drop_add without partials; the f32
(generic) depthwise kernels and accumulate 1 of ewvit_dwconv3x3_bwd_weight; ewvit_se_reduce,
ewvit_se_mlp_fwd, ewvit_se_mlp_bwd (no caller); f32 ewvit_se_scale / ewvit_scale_add / max pool.

References are torch fp32 (fp64 for plain sums) on the same bf16-rounded inputs.  Tolerances are
those of test_gpu_bn / test_gpu_se: a bf16 output is one rounding of an fp32 result, 2^-7 of
scale; f32 outputs 1e-4 (BatchNorm: rsqrt / exp ulps) and 1e-5 (SE, depthwise: <= 9-term fp32
sums); gradients and reductions 2e-3 of scale (fp32 sums in another order); bf16 input gradients
2e-2.  Where the header promises the same bits (the partial-statistics forms against the forms
with their own reduction pass, accumulate against overwrite + add, ewvit_se_mlp_fwd against
ewvit_se_squeeze_mlp_fwd) the check is torch.equal.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.bfloat16, torch.float32]
EPS = 1e-3


def _L():
    import ewvit
    return ewvit._lib


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def out_tol(dtype, f32_tol):
    return 2 ** -7 if dtype == torch.bfloat16 else f32_tol


def dx_tol(dtype):
    return 2e-2 if dtype == torch.bfloat16 else 2e-3


def act_ref(z, act):
    return torch.relu(z) if act == 1 else F.silu(z) if act == 2 else z


def nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


# ------------------------------------------------------------------ BatchNorm family
BN_N, BN_HW = 3, 25
BN_M = BN_N * BN_HW          # 75 rows: fewer than a block's row groups, a multiple of nothing


def bn_case(C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(BN_M, C, generator=g) * 1.5 + 0.4).to(dtype)
    dy = torch.randn(BN_M, C, generator=g).to(dtype)
    gamma = torch.randn(C, generator=g) * 0.4 + 1
    beta = torch.randn(C, generator=g) * 0.2
    return x.to(DEV), dy.to(DEV), gamma.to(DEV), beta.to(DEV)


def bn_ref(x, dy_eff, gamma, beta, act, groups):
    """torch fp32 BatchNorm(+act) per row group and its backward for the output gradient dy_eff:
    y, mean, invstd [groups][C], dx, dgamma, dbeta."""
    xr = x.float().clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    xg = xr.view(groups, -1, x.shape[1])
    mean = xg.mean(1, keepdim=True)
    invstd = torch.rsqrt(xg.var(1, unbiased=False, keepdim=True) + EPS)
    y = act_ref((xg - mean) * invstd * gr + br, act).reshape(x.shape)
    y.backward(dy_eff.float())
    return (y.detach(), mean.detach().view(groups, -1).contiguous(), invstd.detach().view(groups, -1).contiguous(),
            xr.grad, gr.grad, br.grad)


def bn_workspace(C, groups):
    L = _L()
    return nan(L.load().ewvit_bn_workspace(BN_M, C, groups) // 4)


def bn_bwd(x, dy, gamma, beta, mean, invstd, act, groups, accumulate=0, dg=None, db=None):
    L = _L()
    C = x.shape[1]
    dx = torch.empty_like(x)
    dg = nan(C) if dg is None else dg
    db = nan(C) if db is None else db
    ws = bn_workspace(C, groups)
    L.call('ewvit_bn_bwd', L.ptr(dy), L.ptr(x), L.ptr(dx), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta), L.ptr(mean),
           L.ptr(invstd), act, L.ptr(dg), L.ptr(db), accumulate, groups, L.ptr(ws), L.stream(x))
    return dx, dg, db


@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bn_fwd_and_partials(dtype, act, C, groups):
    """ewvit_bn_fwd against torch, and ewvit_bn_fwd_partials from the partial rows its statistics
    pass left in the workspace: the same apply pass, so the same bits."""
    L = _L()
    x, dy, gamma, beta = bn_case(C, dtype, 11 * C + groups)
    yr, mr, ir, *_ = bn_ref(x, dy, gamma, beta, act, groups)
    outs = []
    nrc = int(L.load().ewvit_bn_bwd_reduce_rows(BN_M, C, groups))
    assert nrc == 1
    ws = bn_workspace(C, groups)
    for partials in (False, True):
        y = torch.empty_like(x)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        mean, invstd = nan(groups, C), nan(groups, C)
        cnt = torch.zeros((), dtype=torch.int64, device=DEV)
        if not partials:
            L.call('ewvit_bn_fwd', L.ptr(x), L.ptr(y), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv),
                   1, 0.1, EPS, act, L.ptr(mean), L.ptr(invstd), groups, L.ptr(cnt), L.ptr(ws), L.stream(x))
        else:
            part, shifts = ws[:groups * nrc * 2 * C], ws[groups * nrc * 2 * C:]
            L.call('ewvit_bn_fwd_partials', L.ptr(x), L.ptr(y), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta), L.ptr(rm),
                   L.ptr(rv), 0.1, EPS, act, L.ptr(mean), L.ptr(invstd), L.ptr(cnt), L.ptr(part), L.ptr(shifts), nrc,
                   groups, L.stream(x))
        torch.cuda.synchronize()
        assert int(cnt) == groups
        outs.append((y, mean, invstd, rm, rv))
    y, mean, invstd, rm, rv = outs[0]
    assert rel(y.float(), yr) < out_tol(dtype, 1e-4)
    assert rel(mean, mr) < 1e-4 and rel(invstd, ir) < 1e-4
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bn_bwd_accumulate_and_reduce_partials(dtype, act, C, groups):
    """ewvit_bn_bwd against torch; accumulate = 1 adds the same sums to dgamma / dbeta; and
    ewvit_bn_bwd_reduce + ewvit_bn_bwd_partials are ewvit_bn_bwd's two launches: the same bits."""
    L = _L()
    x, dy, gamma, beta = bn_case(C, dtype, 13 * C + groups + act)
    _, mean, invstd, dxr, dgr, dbr = bn_ref(x, dy, gamma, beta, act, groups)
    dx0, dg0, db0 = bn_bwd(x, dy, gamma, beta, mean, invstd, act, groups)
    torch.cuda.synchronize()
    keep = torch.ones_like(dxr, dtype=torch.bool)
    if act == 1:     # away from the ReLU kink (test_gpu_bn): the two sides of z = 0 differ by dy * k
        z = ((x.float().view(groups, -1, C) - mean[:, None]) * invstd[:, None] * gamma + beta).view(BN_M, C)
        keep = z.abs() > 1e-5 * float(z.abs().max())
    assert rel(dx0.float()[keep], dxr[keep]) < dx_tol(dtype)
    assert rel(dg0, dgr) < 2e-3 and rel(db0, dbr) < 2e-3
    g = torch.Generator().manual_seed(C)
    ig, ib = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    dx1, dg1, db1 = bn_bwd(x, dy, gamma, beta, mean, invstd, act, groups, 1, ig.clone(), ib.clone())
    torch.cuda.synchronize()
    assert torch.equal(dx1, dx0) and torch.equal(dg1, ig + dg0) and torch.equal(db1, ib + db0)
    nrc = int(L.load().ewvit_bn_bwd_reduce_rows(BN_M, C, groups))
    part = nan(groups, nrc, 2 * C)
    L.call('ewvit_bn_bwd_reduce', L.ptr(dy), L.ptr(x), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta), L.ptr(mean),
           L.ptr(invstd), act, groups, L.ptr(part), L.stream(x))
    dx2, dg2, db2 = torch.empty_like(x), nan(C), nan(C)
    L.call('ewvit_bn_bwd_partials', L.ptr(dy), L.ptr(x), L.ptr(dx2), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta),
           L.ptr(mean), L.ptr(invstd), act, L.ptr(dg2), L.ptr(db2), None, 1, L.ptr(part), nrc, groups, L.stream(x))
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx0) and torch.equal(dg2, dg0) and torch.equal(db2, db0)


@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bn_bwd_scaled_and_partials_row_scale(dtype, C):
    L = _L()
    x, dy, gamma, beta = bn_case(C, dtype, 17 * C)
    rs = torch.tensor([1 / 0.7, 0.0, 1 / 0.7], device=DEV)
    dy_eff = dy.float() * rs.repeat_interleave(BN_HW)[:, None]
    _, mean, invstd, dxr, dgr, dbr = bn_ref(x, dy_eff, gamma, beta, 0, 1)
    dx, dg, db = torch.empty_like(x), nan(C), nan(C)
    ws = bn_workspace(C, 1)
    L.call('ewvit_bn_bwd_scaled', L.ptr(dy), L.ptr(x), L.ptr(dx), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta),
           L.ptr(mean), L.ptr(invstd), L.ptr(dg), L.ptr(db), L.ptr(rs), BN_HW, L.ptr(ws), L.stream(x))
    torch.cuda.synchronize()
    assert rel(dx.float(), dxr) < dx_tol(dtype)
    assert rel(dg, dgr) < 2e-3 and rel(db, dbr) < 2e-3
    # the dx pass alone from the partial rows the reduction pass left in the workspace: same bits
    nrc = int(L.load().ewvit_bn_bwd_reduce_rows(BN_M, C, 1))
    dx2, dg2, db2 = torch.empty_like(x), nan(C), nan(C)
    L.call('ewvit_bn_bwd_partials', L.ptr(dy), L.ptr(x), L.ptr(dx2), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta),
           L.ptr(mean), L.ptr(invstd), 0, L.ptr(dg2), L.ptr(db2), L.ptr(rs), BN_HW, L.ptr(ws), nrc, 1, L.stream(x))
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)


@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bn_bwd_se(dtype, act, C):
    L = _L()
    x, dy, gamma, beta = bn_case(C, dtype, 19 * C + act)
    g = torch.Generator().manual_seed(C + act)
    se_s = torch.rand(BN_N, C, generator=g).to(DEV)
    se_g = (torch.randn(BN_N, C, generator=g) * 0.05).to(DEV)
    dy_eff = dy.float() * se_s.repeat_interleave(BN_HW, 0) + se_g.repeat_interleave(BN_HW, 0)
    _, mean, invstd, dxr, dgr, dbr = bn_ref(x, dy_eff, gamma, beta, act, 1)
    dx, dg, db = torch.empty_like(x), nan(C), nan(C)
    ws = bn_workspace(C, 1)
    L.call('ewvit_bn_bwd_se', L.ptr(dy), L.ptr(x), L.ptr(dx), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta), L.ptr(mean),
           L.ptr(invstd), act, L.ptr(dg), L.ptr(db), L.ptr(se_s), L.ptr(se_g), BN_HW, L.ptr(ws), L.stream(x))
    torch.cuda.synchronize()
    keep = torch.ones_like(dxr, dtype=torch.bool)
    if act == 1:
        z = (x.float() - mean) * invstd * gamma + beta
        keep = z.abs() > 1e-5 * float(z.abs().max())
    assert rel(dx.float()[keep], dxr[keep]) < dx_tol(dtype)
    assert rel(dg, dgr) < 2e-3 and rel(db, dbr) < 2e-3


@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bn_fwd_drop_add_own_statistics(dtype, C):
    """part == NULL: the statistics pass runs inside the call; against torch with the factors the
    kernel drew, and bit-equal to the call given the partial rows of ewvit_bn_fwd's statistics pass."""
    L = _L()
    x, skip, gamma, beta = bn_case(C, dtype, 23 * C)
    keep = 0.6
    outs = []
    nrc = int(L.load().ewvit_bn_bwd_reduce_rows(BN_M, C, 1))
    for partials in (False, True):
        ws = bn_workspace(C, 1)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        part = shifts = None
        if partials:
            y0 = torch.empty_like(x)
            L.call('ewvit_bn_fwd', L.ptr(x), L.ptr(y0), L.dt(x), BN_M, C, None, None, None, None, 1, 0.1, EPS, 0, None,
                   None, 1, None, L.ptr(ws), L.stream(x))
            part, shifts = ws[:nrc * 2 * C], ws[nrc * 2 * C:]
        y = torch.empty_like(x)
        mean, invstd, scale = nan(C), nan(C), nan(BN_N)
        cnt = torch.zeros((), dtype=torch.int64, device=DEV)
        L.call('ewvit_bn_fwd_drop_add', L.ptr(x), L.ptr(y), L.dt(x), BN_M, C, L.ptr(gamma), L.ptr(beta), L.ptr(rm),
               L.ptr(rv), 0.1, EPS, L.ptr(mean), L.ptr(invstd), L.ptr(cnt), L.ptr(part), L.ptr(shifts),
               nrc if partials else 0, L.ptr(skip), BN_HW, keep, 12345, None, L.ptr(scale),
               None if partials else L.ptr(ws), L.stream(x))
        torch.cuda.synchronize()
        assert int(cnt) == 1
        outs.append((y, mean, invstd, scale, rm, rv))
    y, mean, invstd, scale, rm, rv = outs[0]
    assert all(v == 0.0 or abs(v - 1 / keep) < 1e-6 for v in scale.cpu().tolist())
    yr, mr, ir, *_ = bn_ref(x, skip, gamma, beta, 0, 1)
    ref = yr * scale.repeat_interleave(BN_HW)[:, None] + skip.float()
    assert rel(y.float(), ref) < out_tol(dtype, 1e-4)
    assert rel(mean, mr[0]) < 1e-4 and rel(invstd, ir[0]) < 1e-4
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ depthwise 3x3
DW_N, DW_H = 2, 5


def dw_case(C, dtype, stride, seed):
    g = torch.Generator().manual_seed(seed)
    Ho = (DW_H - 1) // stride + 1
    x = torch.randn(DW_N, C, DW_H, DW_H, generator=g).to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(DW_N, C, Ho, Ho, generator=g).to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(C, 1, 3, 3, generator=g) * 0.3).to(DEV).contiguous()
    return x, dy, w, Ho


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('dtype', DTYPES)
def test_dwconv_fwd_bwd_data_bwd_weight(dtype, C, stride):
    """bf16 takes the row kernels, f32 the generic ones; accumulate = 1 adds the same dW."""
    L = _L()
    x, dy, w, Ho = dw_case(C, dtype, stride, 29 * C + stride)
    xr, wr = x.float().cpu().requires_grad_(True), w.cpu().requires_grad_(True)     # fp32 on the CPU
    yr = F.conv2d(xr, wr, None, stride, 1, 1, C)
    yr.backward(dy.float().cpu())
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    L.call('ewvit_dwconv3x3_fwd', L.ptr(x), L.ptr(w), L.ptr(y), DW_N, DW_H, DW_H, C, stride, 1, L.dt(x), L.stream(x))
    L.call('ewvit_dwconv3x3_bwd_data', L.ptr(dy), L.ptr(w), L.ptr(dx), DW_N, DW_H, DW_H, C, stride, 1, L.dt(x),
           L.stream(x))
    ws = nan(L.load().ewvit_dwconv3x3_bwd_weight_workspace(DW_N, DW_H, DW_H, C, stride, 1) // 4)
    g = torch.Generator().manual_seed(C)
    init = torch.randn(C, 1, 3, 3, generator=g).to(DEV)
    dw0, dw1 = nan(C, 1, 3, 3), init.clone()
    for dw, acc in ((dw0, 0), (dw1, 1)):
        L.call('ewvit_dwconv3x3_bwd_weight', L.ptr(x), L.ptr(dy), L.ptr(dw), acc, DW_N, DW_H, DW_H, C, stride, 1,
               L.dt(x), L.ptr(ws), L.stream(x))
    torch.cuda.synchronize()
    assert rel(y.float(), yr) < out_tol(dtype, 1e-5)
    assert rel(dx.float(), xr.grad) < out_tol(dtype, 1e-5)
    assert rel(dw0, wr.grad) < 2e-3
    assert torch.equal(dw1, init + dw0)


def _sums(part, C):
    p = part.double().sum(0)
    return p[:C], p[C:]


@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('act', [0, 1, 2])
def test_dwconv_bwd_fused(act, C):
    """ewvit_dwconv3x3_bwd_fused against ewvit_dwconv3x3_bwd_data_bn + ewvit_dwconv3x3_bwd_weight
    (test_gpu_bn_link): dx bit-exact, the BatchNorm sums of both against the fp64 sums of the
    stored dx (1e-5 of the sum of magnitudes), dW within 1e-5 of its largest entry."""
    L = _L()
    x, dy, w, _ = dw_case(C, torch.bfloat16, 1, 31 * C + act)
    g = torch.Generator().manual_seed(C + act)
    bx = (torch.randn(DW_N, C, DW_H, DW_H, generator=g) * 1.5 + 0.3).to(torch.bfloat16).to(DEV).contiguous(
        memory_format=torch.channels_last)
    gamma = (torch.randn(C, generator=g) * 0.3 + 1).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    mean = bx.float().mean((0, 2, 3)).contiguous()
    invstd = torch.rsqrt(bx.float().var((0, 2, 3), unbiased=False) + EPS).contiguous()
    nrc = int(L.load().ewvit_dwconv3x3_bn_rows(DW_N, DW_H, DW_H, C, 1, 1))
    assert nrc == 1
    dx0, dx1 = torch.empty_like(x), torch.empty_like(x)
    part0, part1 = nan(nrc, 2 * C), nan(nrc, 2 * C)
    L.call('ewvit_dwconv3x3_bwd_data_bn', L.ptr(dy), L.ptr(w), L.ptr(dx0), DW_N, DW_H, DW_H, C, L.ptr(bx), L.ptr(mean),
           L.ptr(invstd), L.ptr(gamma), L.ptr(beta), act, L.ptr(part0), L.stream(x))
    ws0 = nan(L.load().ewvit_dwconv3x3_bwd_weight_workspace(DW_N, DW_H, DW_H, C, 1, 1) // 4)
    dw0, dw1 = nan(C, 1, 3, 3), nan(C, 1, 3, 3)
    L.call('ewvit_dwconv3x3_bwd_weight', L.ptr(x), L.ptr(dy), L.ptr(dw0), 0, DW_N, DW_H, DW_H, C, 1, 1, L.BF16,
           L.ptr(ws0), L.stream(x))
    ws1 = nan(L.load().ewvit_dwconv3x3_bwd_fused_workspace(DW_N, DW_H, DW_H, C) // 4)
    L.call('ewvit_dwconv3x3_bwd_fused', L.ptr(dy), L.ptr(w), L.ptr(dx1), L.ptr(x), L.ptr(dw1), 0, DW_N, DW_H, DW_H, C,
           L.ptr(bx), L.ptr(mean), L.ptr(invstd), L.ptr(gamma), L.ptr(beta), act, L.ptr(part1), L.ptr(ws1),
           L.stream(x))
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1)
    v = lambda t: t.double().view(1, C, 1, 1)
    xh = (bx.double() - v(mean)) * v(invstd)
    z = xh * v(gamma) + v(beta)
    sg = torch.sigmoid(z)
    gr = dx1.double() * ((z > 0).double() if act == 1 else sg * (1 + z * (1 - sg)) if act == 2 else 1.0)
    ra, rb = gr.sum((0, 2, 3)), (gr * xh).sum((0, 2, 3))
    ma, mb = gr.abs().sum((0, 2, 3)), (gr * xh).abs().sum((0, 2, 3))
    for part in (part0, part1):
        pa, pb = _sums(part, C)
        assert float(((pa - ra).abs() / (ma + 1e-30)).max()) < 1e-5
        assert float(((pb - rb).abs() / (mb + 1e-30)).max()) < 1e-5
    assert float((dw1 - dw0).abs().max()) < 1e-5 * float(dw0.abs().max())


# ------------------------------------------------------------------ squeeze-excitation
SE_N, SE_HW, SE_C, SE_CSQ = 3, 9, 72, 6      # two 64-channel chunks, the second ragged


@pytest.mark.parametrize('N,HW,C', [(SE_N, SE_HW, SE_C), (2, 1024, 64)])     # one split; four splits + the fold
@pytest.mark.parametrize('prod', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_se_reduce(dtype, prod, N, HW, C):
    L = _L()
    g = torch.Generator().manual_seed(HW + C)
    a = torch.randn(N, HW, C, generator=g).to(dtype).to(DEV)
    b = torch.randn(N, HW, C, generator=g).to(dtype).to(DEV) if prod else None
    wsb = int(L.load().ewvit_se_reduce_workspace(N, HW, C))
    assert wsb == (4 if HW == 1024 else 1) * N * C * 4
    ws, out = nan(wsb // 4), nan(N, C)
    scale = 1.0 if prod else 1.0 / HW
    L.call('ewvit_se_reduce', L.ptr(a), L.ptr(b), L.dt(a), N, HW, C, scale, L.ptr(out), L.ptr(ws), L.stream(a))
    torch.cuda.synchronize()
    ref = ((a.double() * b.double()) if prod else a.double()).sum(1) * scale
    assert rel(out, ref) < 2e-3


def se_weights(seed):
    g = torch.Generator().manual_seed(seed)
    w1 = (torch.randn(SE_CSQ, SE_C, generator=g) * 0.2).to(DEV)
    b1 = (torch.randn(SE_CSQ, generator=g) * 0.1).to(DEV)
    w2 = (torch.randn(SE_C, SE_CSQ, generator=g) * 0.3).to(DEV)
    b2 = (torch.randn(SE_C, generator=g) * 0.1).to(DEV)
    return w1, b1, w2, b2


@pytest.mark.parametrize('dtype', DTYPES)
def test_se_mlp_fwd_and_bwd(dtype):
    """ewvit_se_mlp_fwd from the s0 ewvit_se_squeeze_mlp_fwd wrote: h1 and s bit for bit ("exactly
    as", ewvit.h); ewvit_se_mlp_bwd fed ds = ewvit_se_reduce(dy, x) against torch autograd of
    y = x * sigmoid(W2 silu(W1 mean_hw(x) + b1) + b2)."""
    L = _L()
    N, HW, C, Csq = SE_N, SE_HW, SE_C, SE_CSQ
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, HW, C, generator=g).to(dtype).to(DEV)
    dy = torch.randn(N, HW, C, generator=g).to(dtype).to(DEV)
    w1, b1, w2, b2 = se_weights(8)
    fws = nan(L.load().ewvit_se_mlp_fwd_workspace(N, C, Csq) // 4)
    s0, h1, s = nan(N, C), nan(N, Csq), nan(N, C)
    L.call('ewvit_se_squeeze_mlp_fwd', L.ptr(x), L.dt(x), N, HW, C, L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), Csq,
           L.ptr(s0), L.ptr(h1), L.ptr(s), L.ptr(fws), L.stream(x))
    fws2 = nan(fws.numel())
    h1b, sb = nan(N, Csq), nan(N, C)
    L.call('ewvit_se_mlp_fwd', L.ptr(s0), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(h1b), L.ptr(sb), N, C, Csq,
           L.ptr(fws2), L.stream(x))
    torch.cuda.synchronize()
    assert torch.equal(h1, h1b) and torch.equal(s, sb)
    xr = x.float().cpu().requires_grad_(True)                                        # fp32 on the CPU
    pr = [p.cpu().requires_grad_(True) for p in (w1, b1, w2, b2)]
    s0r = xr.mean(1)
    s0r.retain_grad()
    h1r = s0r @ pr[0].t() + pr[1]
    sr = torch.sigmoid(F.silu(h1r) @ pr[2].t() + pr[3])
    (xr * sr[:, None, :]).backward(dy.float().cpu())
    assert rel(s0, s0r) < 1e-5 and rel(h1, h1r) < 1e-5 and rel(s, sr) < 1e-5
    ds = nan(N, C)
    rws = nan(L.load().ewvit_se_reduce_workspace(N, HW, C) // 4)
    L.call('ewvit_se_reduce', L.ptr(dy), L.ptr(x), L.dt(x), N, HW, C, 1.0, L.ptr(ds), L.ptr(rws), L.stream(x))
    bws = nan(L.load().ewvit_se_mlp_bwd_workspace(N, C, Csq) // 4)
    gq, dw1, db1, dw2, db2 = nan(N, C), nan(Csq, C), nan(Csq), nan(C, Csq), nan(C)
    L.call('ewvit_se_mlp_bwd', L.ptr(ds), L.ptr(s), L.ptr(h1), L.ptr(s0), L.ptr(w1), L.ptr(w2), 1.0 / HW, L.ptr(gq),
           L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(db2), N, C, Csq, L.ptr(bws), L.stream(x))
    torch.cuda.synchronize()
    assert rel(gq, s0r.grad / HW) < 2e-3
    for got, p in zip((dw1, db1, dw2, db2), pr):
        assert rel(got, p.grad) < 2e-3
    # and the squeeze's share of dx through ewvit_se_scale: dx = dy * s + g
    dx = torch.empty_like(x)
    L.call('ewvit_se_scale', L.ptr(dy), L.dt(x), L.ptr(s), L.ptr(gq), L.ptr(dx), N, HW, C, L.stream(x))
    torch.cuda.synchronize()
    assert rel(dx.float(), xr.grad) < dx_tol(dtype)


@pytest.mark.parametrize('with_g', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_se_scale(dtype, with_g):
    L = _L()
    N, HW, C = SE_N, SE_HW, SE_C
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N, HW, C, generator=g).to(dtype).to(DEV)
    s = torch.rand(N, C, generator=g).to(DEV)
    gg = torch.randn(N, C, generator=g).to(DEV) if with_g else None
    y = torch.empty_like(x)
    L.call('ewvit_se_scale', L.ptr(x), L.dt(x), L.ptr(s), L.ptr(gg), L.ptr(y), N, HW, C, L.stream(x))
    torch.cuda.synchronize()
    ref = x.float() * s[:, None, :] + (gg[:, None, :] if with_g else 0)
    assert rel(y.float(), ref) < out_tol(dtype, 1e-5)


@pytest.mark.parametrize('with_x', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_scale_add(dtype, with_x):
    L = _L()
    N, E = 3, 9 * 72
    g = torch.Generator().manual_seed(10)
    r = torch.randn(N, E, generator=g).to(dtype).to(DEV)
    x = torch.randn(N, E, generator=g).to(dtype).to(DEV) if with_x else None
    sc = torch.tensor([1.25, 0.0, 1.25], device=DEV)
    y = torch.empty_like(r)
    L.call('ewvit_scale_add', L.ptr(r), L.ptr(x), L.dt(r), L.ptr(sc), L.ptr(y), N, E, L.stream(r))
    torch.cuda.synchronize()
    ref = r.float() * sc[:, None] + (x.float() if with_x else 0)
    assert rel(y.float(), ref) < out_tol(dtype, 1e-5)


@pytest.mark.parametrize('dtype', DTYPES)
def test_maxpool2_odd_side(dtype):
    """N = 1, H = W = 5, C = 8: the floor-mode remainder row / column gets no output and dx = 0."""
    L = _L()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 8, 5, 5, generator=g).to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(1, 8, 2, 2, generator=g).to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)
    y = torch.empty_like(dy)
    arg = torch.full((1, 2, 2, 8), 255, dtype=torch.uint8, device=DEV)
    dx = torch.full_like(x, float('nan'))
    L.call('ewvit_maxpool2_fwd', L.ptr(x), L.ptr(y), L.ptr(arg), L.dt(x), 1, 5, 5, 8, L.stream(x))
    L.call('ewvit_maxpool2_bwd', L.ptr(dy), L.ptr(arg), L.ptr(dx), L.dt(x), 1, 5, 5, 8, L.stream(x))
    torch.cuda.synchronize()
    xr = x.float().cpu().requires_grad_(True)
    yr = F.max_pool2d(xr, 2)
    yr.backward(dy.float().cpu())
    assert torch.equal(y.float().cpu(), yr) and torch.equal(dx.float().cpu(), xr.grad)

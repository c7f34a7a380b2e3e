"""Float64 references for the generic token kernels (a helper module, not a test).

csrc/gemm.hip (ewvit_gemm, ewvit_gemm_mx8, ewvit_act_bwd, ewvit_dropout_bwd, ewvit_colsum),
csrc/layernorm.hip, csrc/attention.hip and the tall-K GEMM at the end of csrc/vit.hip, restated
in float64 on plain CPU tensors, plus the deterministic inputs that tests/test_gpu_token_ops.py
feeds the kernels and the bounds it holds them to.  tests/test_token_ref_cpu.py proves the
references against torch float64 and shows that every bound rejects a deliberately wrong result
built from the same inputs.

Operands are given in their logical orientation (A [M, K], B [K, N]) whatever their storage
order; `place` lays a logical operand out K-contiguous or K-strided inside a wider buffer, so
the same values reach every staging path of the kernels.

Dropout enters as an explicit 0/1 mask with its p.  Nothing here generates the kernels' random
numbers: the GPU tests read the mask back from the library (ewvit_dropout_bwd on ones).

Nothing in this module calls into ewvit.
"""
import functools
import math

import torch

from fused_ref import layernorm as layernorm_ref          # noqa: F401  (torch's formula, float64)
from fused_ref import layernorm_bwd as layernorm_bwd_ref  # noqa: F401

F64 = torch.float64

# ---------------------------------------------------------------- bounds (of scale)
GEMM_PLAIN = 2e-4        # f32 output, no epilogue: summation order only (tests/test_gpu_kernels.py)
GEMM_EPI = 5e-4          # f32 output behind an epilogue
BF16_OUT = 2.0 ** -7     # a bf16 output, and the bf16 pre-activation `aux`
MX_ROW = 1e-4            # MXFP8 product, per output row (test_fp8_gemm_vs_torch_e4m3_emulation)
ACT_BWD_GELU = 1e-6      # f32 GELU' (erff + exp) against float64
COLSUM = 1e-5
TALLK = 1e-4
LN_F32 = 2e-5
ATTN_FWD, ATTN_GRAD = 1e-2, 1.5e-2
ATTN_P_SUM, ATTN_P = 1e-6, 1e-5
RELU_ZERO = 1e-5         # act 2: elements with |pre| within this of scale of zero are left out
RELU_CAP = 1e-3          # ... at most this fraction of them


# ---------------------------------------------------------------- rounding
def bf16(x):
    return x.float().bfloat16().to(F64)


def mxq(x):
    """MXFP8 of x [R, K] along K in float64 (`_mx_q` of tests/test_gpu_fp8.py, which is pinned
    bit-level against ewvit_gemm_mx8)."""
    from test_gpu_fp8 import _mx_q
    return _mx_q(x.float()).to(F64)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_erf_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def drop_scale(p):
    """1 / (1 - p) as the kernels form it: one f32 division."""
    one = torch.ones((), dtype=torch.float32)
    return float(one / (one - torch.tensor(p, dtype=torch.float32)))


# ---------------------------------------------------------------- GEMM
def gemm_ref(A, B, *, rounding='bf16', alpha=1.0, beta=0.0, C0=None, bias=None, act=0, aux=None, mask=None,
             p=0.0, resid=None):
    """epilogue(alpha A B) in the order of `epilogue()` in csrc/gemm.hip -> (y, pre).

    A [M, K], B [K, N]; rounding 'bf16' (both operands rounded to bf16) or 'mx' (MXFP8 blocks of
    32 along K).  v = alpha acc + bias (`pre`; the kernel stores bf16(v) as aux for act 1/2);
    act 1 GELU(erf), 2 ReLU, 3 v GELU'(aux) with `aux` the stored pre-activation of an earlier
    launch; then mask / (1 - p), + resid, + beta C0."""
    if rounding == 'bf16':
        acc = bf16(A) @ bf16(B)
    else:
        assert rounding == 'mx', rounding
        acc = mxq(A) @ mxq(B.t()).t()
    v = alpha * acc
    if bias is not None:
        v = v + bias.to(F64)
    pre = v
    if act == 1:
        v = gelu_erf(v)
    elif act == 2:
        v = torch.relu(v)
    elif act == 3:
        v = v * gelu_erf_grad(aux.to(F64))
    else:
        assert act == 0, act
    if mask is not None:
        v = v * mask.to(F64) * drop_scale(p)
    if resid is not None:
        v = v + resid.to(F64)
    if beta != 0.0:
        v = v + beta * C0.to(F64)
    return v, pre


def act_bwd_ref(dy, aux, act, mask, p):
    """dy keep / (1 - p) act'(aux): the backward of the GEMM epilogue (act_bwd_kernel)."""
    v = dy.to(F64)
    if mask is not None:
        v = v * mask.to(F64) * drop_scale(p)
    if act == 1:
        v = v * gelu_erf_grad(aux.to(F64))
    elif act == 2:
        v = torch.where(aux.to(F64) > 0, v, torch.zeros_like(v))
    return v


# ---------------------------------------------------------------- attention
def attn_ref(q, k, v, scale):
    """q [B, H, nq, d], k / v [B, H, nk, d] -> (o [B, H, nq, d], p [B, H, nq, nk])."""
    p = torch.softmax(q.to(F64) @ k.to(F64).transpose(-1, -2) * scale, -1)
    return p @ v.to(F64), p


def attn_bwd_ref(do, q, k, v, p, scale):
    """-> dq, dk, dv from the softmax weights p (hand-derived, checked against autograd)."""
    do, q, k, v = (t.to(F64) for t in (do, q, k, v))
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    return ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do


def heads_of(t, H, d):
    """[B, n, H d] -> [B, H, n, d]"""
    B, n, _ = t.shape
    return t.reshape(B, n, H, d).transpose(1, 2)


def tokens_of(t):
    """[B, H, n, d] -> [B, n, H d]"""
    B, H, n, d = t.shape
    return t.transpose(1, 2).reshape(B, n, H * d)


# ---------------------------------------------------------------- comparison
def err_of_scale(got, ref, per_row=False):
    """max |got - ref| / max |ref|; per_row: the largest such ratio over the rows of a matrix,
    each against its own row's scale.  0 / 0 counts as 0, x / 0 as inf."""
    got, ref = torch.as_tensor(got).detach().cpu().to(F64), torch.as_tensor(ref).detach().cpu().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    if per_row:
        err, scale = (got - ref).abs().reshape(ref.shape[0], -1).amax(1), ref.abs().reshape(ref.shape[0], -1).amax(1)
    else:
        err, scale = (got - ref).abs().max().reshape(1), ref.abs().max().reshape(1)
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0).to(F64))
    return float(r.max())


# ---------------------------------------------------------------- layouts
def ld_for(n, aligned):
    """A leading dimension > n: a multiple of 8 (16-byte rows in f32 and bf16: vector staging) or
    3 past one (scalar staging in both types)."""
    return (n + 7) // 8 * 8 + (8 if aligned else 11)


def place(X, kcontig, dtype, aligned=True, fill=float('nan'), device=None):
    """The logical operand X [R, K] stored inside a wider `fill`ed buffer: K-contiguous
    ([R][ld], strides (ld, 1)) or K-strided ([K][ld], strides (1, ld)).  -> (a view with X's
    shape and those strides, (stride over R, stride over K))."""
    R, K = X.shape
    if kcontig:
        ld = ld_for(K, aligned)
        buf = torch.full((R, ld), fill, dtype=dtype, device=device)
        view = buf[:, :K]
        strides = (ld, 1)
    else:
        ld = ld_for(R, aligned)
        buf = torch.full((K, ld), fill, dtype=dtype, device=device)
        view = buf[:, :R].t()
        strides = (1, ld)
    view.copy_(X.to(dtype))
    return view, strides


LAYOUTS = {'nt': (True, True), 'nn': (True, False), 'tn': (False, False), 'tt': (False, True)}
"""name -> (A K-contiguous, B K-contiguous): nn.Linear's forward, its input gradient, its weight
gradient, and the remaining combination."""


# ---------------------------------------------------------------- inputs
INT_M = INT_N = (1, 63, 65, 130)
INT_K = ((1, 1), (31, 1), (33, 1), (160, 1), (4096, 1), (4096, 3))     # (K, splitk)


@functools.lru_cache(maxsize=None)
def int_operands():
    """Integers in [-8, 8]: A [130, 4096], B [4096, 130]; a case takes the leading M x K / K x N.
    Every value is exact in bf16 and every partial sum stays below 64 * 4096 = 2^18 < 2^24, so
    the f32-accumulated product is the exact one in any summation order."""
    g = torch.Generator().manual_seed(20)
    return (torch.randint(-8, 9, (130, 4096), generator=g).to(F64), torch.randint(-8, 9, (4096, 130), generator=g).to(F64))


@functools.lru_cache(maxsize=None)
def int_ref(M, N, K):
    A, B = int_operands()
    return A[:M, :K] @ B[:K, :N]


RAND_SHAPE = (70, 93, 200)          # ragged against 64 x 64 x 32 and against the MX K-tile of 128
EPILOGUES = ('plain', 'alpha', 'bias', 'beta1_sk1', 'beta1_sk3', 'betah_sk1', 'betah_sk3', 'gelu_aux_act3', 'relu_aux',
             'resid_f32', 'resid_bf16', 'bf16_c', 'drop_gelu_resid')
P_DROP = 0.15


@functools.lru_cache(maxsize=None)
def rand_case(M, N, K, seed=0, spread=0, adt=torch.float32, bdt=torch.float32):
    """Random operands as the kernels will hold them (already rounded to their storage types):
    A [M, K] ~ 3 N(0, 1), B [K, N] ~ N(0, 1) / sqrt(K), bias, residuals, C0.  spread: every
    32-element K block of every row of A and column of B scaled by its own 10^U(-spread/2,
    spread/2) (`spread = 6` of test_fp8_gemm_vs_torch_e4m3_emulation)."""
    g = torch.Generator().manual_seed(1000 * seed + M + 7 * N + 13 * K + spread)
    A = torch.randn(M, K, generator=g) * 3
    B = torch.randn(K, N, generator=g) / K ** 0.5
    if spread:
        nb = (K + 31) // 32
        sa = torch.pow(10.0, (torch.rand(M, nb, generator=g) - 0.5) * spread).repeat_interleave(32, 1)[:, :K]
        sb = torch.pow(10.0, (torch.rand(nb, N, generator=g) - 0.5) * spread).repeat_interleave(32, 0)[:K]
        A, B = A * sa, B * sb
    return {'A': A.to(adt).float(), 'B': B.to(bdt).float(), 'bias': torch.randn(N, generator=g),
            'resid': torch.randn(M, N, generator=g), 'C0': torch.randn(M, N, generator=g),
            'cpu_mask': (torch.rand(M, N, generator=g) >= P_DROP)}


def epilogue_args(name, c, mask=None, aux=None):
    """The reference's keyword arguments of one named epilogue (the GPU test passes the kernel the
    same ones).  -> (kwargs of gemm_ref, splitk, C is bf16)."""
    kw, sk, cb = {}, 1, False
    if name == 'plain':
        pass
    elif name == 'alpha':
        kw = dict(alpha=0.5)
    elif name == 'bias':
        kw = dict(bias=c['bias'])
    elif name.startswith('beta'):
        kw = dict(beta=1.0 if name[4] == '1' else 0.5, C0=c['C0'])
        sk = int(name[-1])
    elif name == 'gelu_aux_act3':
        kw = dict(bias=c['bias'], act=1)
    elif name == 'act3':
        kw = dict(act=3, aux=aux)
    elif name == 'relu_aux':
        kw = dict(bias=c['bias'], act=2)
    elif name == 'resid_f32':
        kw = dict(resid=c['resid'])
    elif name == 'resid_bf16':
        kw = dict(resid=c['resid'].bfloat16().float())
    elif name == 'bf16_c':
        kw, cb = dict(bias=c['bias']), True
    elif name == 'drop_gelu_resid':
        kw = dict(bias=c['bias'], act=1, mask=mask, p=P_DROP, resid=c['resid'])
    else:
        raise KeyError(name)
    return kw, sk, cb


def relu_keep(pre):
    """act 2: the elements compared (|pre| further than RELU_ZERO of scale from zero, where one
    rounding cannot flip the ReLU) and the fraction left out."""
    keep = pre.abs() > RELU_ZERO * float(pre.abs().max())
    return keep, 1.0 - float(keep.double().mean())


MX_SPREAD_SHAPE = (70, 93, 160)     # 5 blocks of 32: one full MX K-tile and a 32-wide tail
MX_KS = ((70, 1), (128, 1), (129, 1), (300, 2))                         # (K, splitk)

ACT_BWD_SHAPE = (37, 65)
COLSUM_M, COLSUM_NS = 301, (1, 64, 65)
TALLK_K, TALLK_N, TALLK_MS = 16384, 256, (1, 17, 64)


@functools.lru_cache(maxsize=None)
def tallk_case():
    g = torch.Generator().manual_seed(77)
    X = torch.randn(64, TALLK_K, generator=g).bfloat16()
    W = torch.randn(TALLK_N, TALLK_K, generator=g) * 0.01
    b = torch.randn(TALLK_N, generator=g)
    ref = X.to(F64) @ bf16(W).t()
    return X, W, b, ref


LN_DS, LN_MS = (1, 63, 64, 65, 1000, 1024), (1, 3, 5)
LN_BIG = (16384 + 5, 96)
LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def ln_case(M, D, xdt=torch.float32, kind='rand'):
    """x [M, D] (as stored), gamma, beta, dy, dx0 (the gradient accumulated onto) and the float64
    results.  kind 'rand': 3 N(0, 1) + 1;  'far': 1000 + N(0, 1);  'const': every row one value
    (0, 1, -2.5, 3.7, 1000.1, ...) — variance 0."""
    g = torch.Generator().manual_seed(31 * M + D + len(kind))
    if kind == 'rand':
        x = torch.randn(M, D, generator=g) * 3 + 1
    elif kind == 'far':
        x = 1000 + torch.randn(M, D, generator=g)
    else:
        vals = torch.tensor([0.0, 1.0, -2.5, 3.7, 1000.1])
        x = vals[torch.arange(M) % 5][:, None].expand(M, D).contiguous()
    x = x.to(xdt).float()
    gm, bt = torch.randn(D, generator=g) + 1.5, torch.randn(D, generator=g)
    dy, dx0 = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    y, mu, rs = layernorm_ref(x.to(F64), gm.to(F64), bt.to(F64), LN_EPS)
    dx, dg, db = layernorm_bwd_ref(dy.to(F64), x.to(F64), mu, rs, gm.to(F64))
    return {'x': x, 'gamma': gm, 'beta': bt, 'dy': dy, 'dx0': dx0, 'y': y, 'mean': mu, 'rstd': rs, 'dx': dx,
            'dgamma': dg, 'dbeta': db}


def ln_far_bound(c):
    """LN_F32 + 2^-23 max|mean| max rstd: the f32 mean of a row carries a rounding error of order
    2^-24 |mean| per addition of its 64-lane tree, every x - mean of the row inherits it, and
    xhat = (x - mean) rstd scales it by rstd = 1 / std.  The centred second pass adds nothing of
    that order; a one-pass E[x^2] - mean^2 loses 2^-24 mean^2 / var instead."""
    return LN_F32 + 2.0 ** -23 * float(c['mean'].abs().max()) * float(c['rstd'].max())


def ln_onepass_f32(x, gamma, beta, eps):
    """The WRONG LayerNorm the far-mean bound exists to catch: var = E[x^2] - mean^2 in f32."""
    x = x.float()
    mu = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mu * mu
    return (x - mu) * torch.rsqrt(var.clamp_min(0) + eps) * gamma.float() + beta.float()


ATTN_D_SWEEP = 32
ATTN_DS = (1, 63, 64, 65, 127, 128)
ATTN_BH = ((1, 1), (5, 1), (7, 3))                                      # (B, H): B H = 1, 5, 21
# (packed, B, H, nq, nk) with logits of order +-100: each reaches |100|; cross and packed each hold
# rows that are one-hot in f32 next to live ones (tests/test_token_ref_cpu.py)
ATTN_BIG = ((False, 7, 3, 8, 8), (False, 7, 3, 8, 4), (True, 7, 3, 8, 8), (True, 7, 3, 2, 2))


@functools.lru_cache(maxsize=None)
def attn_case(packed, B, H, nq, nk, d, big=False):
    """bf16 q [B, nq, H d], k / v [B, nk, H d], do; the float64 results on those bf16 values.
    big: q and k scaled so the logits have a standard deviation of 35 and reach +-100."""
    g = torch.Generator().manual_seed(B + 3 * H + 17 * nq + 131 * nk + 1009 * d + int(packed))
    a = 35.0 ** 0.5 if big else 1.0
    q = (torch.randn(B, nq, H * d, generator=g) * a).bfloat16()
    k = (torch.randn(B, nk, H * d, generator=g) * a).bfloat16()
    v = torch.randn(B, nk, H * d, generator=g).bfloat16()
    do = torch.randn(B, nq, H * d, generator=g).bfloat16()
    scale = d ** -0.5
    qh, kh, vh, doh = (heads_of(t, H, d) for t in (q, k, v, do))
    o, p = attn_ref(qh, kh, vh, scale)
    dq, dk, dv = attn_bwd_ref(doh, qh, kh, vh, p, scale)
    logits = qh.to(F64) @ kh.to(F64).transpose(-1, -2) * scale
    return {'q': q, 'k': k, 'v': v, 'do': do, 'scale': scale, 'o': tokens_of(o), 'p': p, 'dq': tokens_of(dq),
            'dk': tokens_of(dk), 'dv': tokens_of(dv), 'logits': logits}


def one_hot_rows(p):
    """Rows of a float64 softmax that are one-hot in f32: the largest weight rounds to 1 and every
    other one lies below the smallest normal f32."""
    top = p.amax(-1)
    rest = (p * (p < top[..., None])).sum(-1)
    return (top > 1 - 2.0 ** -26) & (rest < 2.0 ** -126)

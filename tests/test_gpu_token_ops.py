"""The generic token kernels over their whole operand matrix, through the C-ABI, against float64.

ewvit_gemm / ewvit_gemm_mx8 / ewvit_act_bwd / ewvit_dropout_bwd / ewvit_colsum (csrc/gemm.hip),
ewvit_gemm_tallk (csrc/vit.hip), ewvit_layernorm_fwd/bwd (csrc/layernorm.hip) and
ewvit_attn_fwd/bwd (csrc/attention.hip): the kernels every model runs on that the fused ViT layer
and DAMA head refuse, everything under torch.compile, patch_to_embedding / feat_map in every
step — and the reference side of every *_matches_module_path test.

The references, the inputs and the bounds live in tests/token_ref.py; tests/test_token_ref_cpu.py
proves the references against torch float64 autograd and shows that each bound below rejects a
wrong result built from these inputs.  Operands sit inside wider NaN-filled buffers (leading
dimensions above the row, once a multiple of 8 — vector staging — and once not), outputs are
slices of wider NaN-filled buffers: a padding element read shows as a NaN inside, an element
written outside a ragged tile as a missing NaN outside.  Dropout masks are read back from the
library (ewvit_dropout_bwd on ones), never regenerated here.  Every measured figure goes through
`log` (EWVIT_PARITY_LOG).

Bounds (max error of the output's scale unless stated) and what the MI355X gave:
kernel / check                         bound                       measured
-------------------------------------  --------------------------  ---------------------------
ewvit_gemm, exact integers             bit-exact (torch.equal)     exact, 4608 launches
ewvit_gemm, f32 C, no epilogue         2e-4                        1.3e-7
ewvit_gemm, f32 C behind an epilogue   5e-4                        1.1e-7 .. 1.8e-7
ewvit_gemm(_mx8), bf16 C and aux       2^-7 = 7.8e-3               2.6e-3 (MX, per row: 3.7e-3)
ewvit_gemm_mx8, f32 C, per output row  1e-4                        2.9e-5 .. 4.6e-5
  every block its own scale            1e-4                        f32 4.3e-5, bf16 6.6e-5
ewvit_act_bwd f32 out, act 0 / 2       bit-exact, exact zeros      exact
ewvit_act_bwd f32 out, GELU'           1e-6                        8.5e-8 .. 1.2e-7
ewvit_act_bwd / dropout_bwd bf16 out   2^-7                        1.9e-3 .. 2.5e-3
ewvit_dropout_bwd f32                  bit-exact                   exact
ewvit_colsum                           1e-5                        0 .. 2.7e-7
ewvit_gemm_tallk vs float64            1e-4                        1.0e-7 .. 2.5e-7
ewvit_gemm_tallk vs ewvit_gemm         1e-4                        1.4e-7 .. 3.0e-7
ewvit_layernorm_fwd/bwd, f32           2e-5                        0 .. 1.9e-7 (M = 16389: 9.2e-7)
ewvit_layernorm_fwd, bf16 y            2^-7                        4.7e-4 .. 3.2e-3
  far-mean rows (1000 + N(0, 1))       2e-5 + 2^-23 |mean| rstd    y 1.7e-5 .. 2.7e-5, dgamma
                                       = 1.4e-4 .. 1.5e-4          2.7e-5 .. 3.7e-5, dx 3.7e-6
  constant rows, per row               2e-5 + 8 2^-24 |value| 316  0.13 of it (y), 3e-3 of it (dx)
ewvit_attn_fwd, o (bf16)               1e-2                        1.2e-3 .. 3.7e-3
ewvit_attn_bwd, dq / dk / dv (bf16)    1.5e-2                      1.3e-3 .. 3.9e-3
  saved p, row sums                    1e-6                        0 .. 1.9e-7
  saved p vs float64 softmax           1e-5 (absolute)             0 .. 1.3e-7
  logits +-100: o, dq, dk, dv          1e-2, 1.5e-2                1.9e-3 .. 3.2e-3; one-hot rows exact

No case failed on the MI355X and no kernel was changed.  The tests do reject wrong kernels: a
build with the m-contiguous staging dropping the last row of a ragged group, the residual added
before the dropout, the LDS quantizer's block scale one slot off, act_bwd's mask drawn at the
strided index, colsum ignoring `accumulate`, a one-pass LayerNorm variance and a softmax without
its max subtraction failed 108 of these cases, each mutation in the tests written for it, and
left the 68 cases that run none of the changed code passing.
"""
import functools

import pytest
import torch

import token_ref as tr
from test_gpu_modules import log

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F64 = torch.float64
F32, BF16 = torch.float32, torch.bfloat16
NAN = float('nan')
SEED = 1234


@pytest.fixture(scope='module', autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail('no ROCm GPU visible')
    import ewvit
    ewvit.load_library()


def _L():
    from ewvit import _lib
    return _lib


def _call(name, *args):
    L = _L()
    L.call(name, *args, L.stream(torch.empty(0, device=DEV)))


def _window(M, N, dtype, col0=3, extra=5):
    """An M x N output as a slice of a wider NaN-filled buffer (one row above and below, col0
    columns left, `extra` right): -> (buffer, view)."""
    buf = torch.full((M + 2, col0 + N + extra), NAN, dtype=dtype, device=DEV)
    return buf, buf[1:M + 1, col0:col0 + N]


def _only_window_written(buf, view):
    """Everything outside the view is still NaN and everything inside is finite."""
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    r0 = (view.data_ptr() - buf.data_ptr()) // buf.element_size() // buf.stride(0)
    c0 = (view.data_ptr() - buf.data_ptr()) // buf.element_size() % buf.stride(0)
    inside[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = True
    return bool(torch.isnan(buf[~inside]).all()) and bool(torch.isfinite(buf[inside]).all())


def _guarded(n, dtype, guard=64):
    """n elements followed by `guard` NaNs that must survive: -> (buffer, the n elements)."""
    buf = torch.full((n + guard,), NAN, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _guard_intact(buf, n):
    return bool(torch.isnan(buf[n:]).all()) and bool(torch.isfinite(buf[:n]).all())


def _kernel_mask(M, N, p, seed, off=None):
    """The keep mask of a launch over M x N with (p, seed, seed_offset), as the library itself
    regenerates it; the kept elements carry exactly the f32 factor 1 / (1 - p)."""
    L = _L()
    g = torch.ones(M, N, device=DEV)
    _call('ewvit_dropout_bwd', L.ptr(g), L.F32, M, N, N, p, seed, L.ptr(off))
    keep = g != 0
    assert torch.equal(g[keep], torch.full_like(g[keep], tr.drop_scale(p)))
    frac = float(keep.float().mean())
    assert abs(frac - (1 - p)) < 5 * (p * (1 - p) / (M * N)) ** 0.5 + 1e-9, frac
    return keep.cpu()


def _gemm(layout, A, B, C, *, adt=F32, bdt=F32, a_aligned=True, b_aligned=True, fp8=False, **kw):
    """C = epi(A B) with A [M, K] and B [K, N] placed as `layout` asks, each inside a wider
    NaN-filled buffer."""
    import ewvit
    ak, bk = tr.LAYOUTS[layout]
    M, K = A.shape
    N = B.shape[1]
    Av, sa = tr.place(A, ak, adt, a_aligned, device=DEV)            # strides over (M, K)
    Bv, sb = tr.place(B.t(), bk, bdt, b_aligned, device=DEV)        # strides over (N, K)
    ewvit.ops.gemm(Av, sa, Bv, (sb[1], sb[0]), C, M, N, K, fp8=fp8, **kw)


# ================================================================ a. exact integers, bf16 kernel
@functools.lru_cache(maxsize=None)
def _int_dev():
    A, B = tr.int_operands()
    return A.float().to(DEV), B.float().to(DEV)


@functools.lru_cache(maxsize=None)
def _int_ref_dev(M, N, K):
    return tr.int_ref(M, N, K).float().to(DEV)


@pytest.mark.parametrize('layout', list(tr.LAYOUTS))
@pytest.mark.parametrize('adt,bdt', [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
def test_gemm_exact_integers_every_layout_dtype_and_stride(layout, adt, bdt):
    """Integers in [-8, 8], sums below 2^24: the f32-accumulated bf16 product IS the float64 one,
    so torch.equal is the bound — one misplaced, dropped or doubled element in K = 4096 shows.
    M, N in {1, 63, 65, 130} x K in {1, 31, 33, 160, 4096 (split-K 1 and 3)}, with both operands
    on aligned leading dimensions (vector staging) and with either one on an odd one (mixed
    vector / scalar staging)."""
    Ad, Bd = _int_dev()
    bad = []
    for M in tr.INT_M:
        for N in tr.INT_N:
            for K, sk in tr.INT_K:
                ref = _int_ref_dev(M, N, K)
                for a_al, b_al in ((True, True), (False, True), (True, False)):
                    buf, C = _window(M, N, F32)
                    _gemm(layout, Ad[:M, :K], Bd[:K, :N], C, adt=adt, bdt=bdt, a_aligned=a_al, b_aligned=b_al,
                          splitk=sk)
                    if not (torch.equal(C, ref) and _only_window_written(buf, C)):
                        bad.append((M, N, K, sk, a_al, b_al, float((C - ref).abs().max())))
    assert not bad, bad[:8]


# ================================================================ b. random data against gemm_ref
_RAND_DT = {'nt': (F32, BF16), 'nn': (BF16, F32), 'tn': (BF16, BF16)}


def _check_out(kind, got, ref, fp8, c_bf16, epi, keep=None):
    got, ref = got.detach().cpu().to(F64), ref.clone()
    if keep is not None:
        got, ref = got * keep, ref * keep
    bound = tr.BF16_OUT if c_bf16 else tr.MX_ROW if fp8 else (tr.GEMM_PLAIN if epi == 'plain' else tr.GEMM_EPI)
    err = tr.err_of_scale(got, ref, per_row=fp8)
    log(kind, err, bound)
    assert err <= bound, (kind, err, bound)
    return err


@pytest.mark.parametrize('fp8', [False, True], ids=['bf16', 'mx'])
@pytest.mark.parametrize('layout', ['nt', 'nn', 'tn'])
@pytest.mark.parametrize('epi', tr.EPILOGUES)
def test_gemm_epilogues_vs_float64(fp8, layout, epi):
    """Both kernels, NT / NN / TN, every epilogue: alpha = 0.5, beta in {1, 0.5} x split-K {1, 3},
    bias, GELU / ReLU with aux, act 3 reading the aux the kernel itself stored, f32 and bf16
    residual with ldr > N, bf16 C, dropout 0.15 with GELU and a residual under the kernel's own
    mask.  bf16 kernel: 2e-4 plain, 5e-4 behind an epilogue; bf16 C and aux 2^-7; MX: per output
    row 1e-4 (2^-7 for bf16)."""
    L = _L()
    M, N, K = tr.RAND_SHAPE
    adt, bdt = _RAND_DT[layout]
    c = tr.rand_case(M, N, K, adt=adt, bdt=bdt)
    rounding = 'mx' if fp8 else 'bf16'
    mask = _kernel_mask(M, N, tr.P_DROP, SEED) if epi == 'drop_gelu_resid' else None
    kw, sk, c_bf16 = tr.epilogue_args(epi, c, mask=mask)
    ref, pre = tr.gemm_ref(c['A'], c['B'], rounding=rounding, **kw)
    buf, C = _window(M, N, BF16 if c_bf16 else F32)
    run = dict(adt=adt, bdt=bdt, b_aligned=layout != 'nn', fp8=fp8, splitk=sk,
               alpha=kw.get('alpha', 1.0), beta=kw.get('beta', 0.0), act=kw.get('act', 0))
    if 'C0' in kw:
        C.copy_(kw['C0'])
    if 'bias' in kw:
        run['bias'] = kw['bias'].to(DEV)
    abuf = aux = rbuf = None
    if kw.get('act') in (1, 2):
        abuf, aux = _window(M, N, BF16)
        assert aux.stride(0) == C.stride(0)                 # aux shares ldc
        run['aux'] = aux
    if 'resid' in kw:
        rbuf, R = _window(M, N, BF16 if epi == 'resid_bf16' else F32, col0=1, extra=6)
        R.copy_(kw['resid'])
        run.update(resid=R, ldr=R.stride(0))
    if mask is not None:
        run.update(drop_p=tr.P_DROP, seed=SEED)
    _gemm(layout, c['A'], c['B'], C, **run)
    assert _only_window_written(buf, C)
    tag = f'gemm_{rounding}_{layout}_{epi}'
    keep = None
    if kw.get('act') == 2:
        keep, left_out = tr.relu_keep(pre)
        assert left_out <= tr.RELU_CAP
    _check_out(tag, C, ref, fp8, c_bf16, epi, keep)
    if mask is not None:
        # a dropped element is the residual alone, to the bit
        assert torch.equal(C.cpu()[~mask], c['resid'][~mask])
    if aux is not None:
        assert _only_window_written(abuf, aux)
        e = tr.err_of_scale(aux.float().cpu(), pre, per_row=fp8)
        log(tag + '_aux', e, tr.BF16_OUT)
        assert e <= tr.BF16_OUT, e
    if epi == 'gelu_aux_act3':
        kw3, _, _ = tr.epilogue_args('act3', c, aux=aux.cpu())
        ref3, _ = tr.gemm_ref(c['A'], c['B'], rounding=rounding, **kw3)
        buf3, C3 = _window(M, N, F32)
        _gemm(layout, c['A'], c['B'], C3, adt=adt, bdt=bdt, fp8=fp8, act=3, aux=aux)
        assert _only_window_written(buf3, C3)
        _check_out(f'gemm_{rounding}_{layout}_act3', C3, ref3, fp8, False, 'act3')


@pytest.mark.parametrize('layout', ['nt', 'nn', 'tn'])
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_mx_every_block_its_own_scale(layout, dt):
    """Every 32-K block of every row of A and column of B under its own 10^U(-3, 3): the E8M0
    scales must follow the blocks in the register path (store_mx) and in the LDS path (quant) of
    NN's B and TN's A and B alike.  Per output row, 1e-4."""
    M, N, K = tr.MX_SPREAD_SHAPE
    c = tr.rand_case(M, N, K, spread=6, adt=dt, bdt=dt)
    ref, _ = tr.gemm_ref(c['A'], c['B'], rounding='mx')
    buf, C = _window(M, N, F32)
    _gemm(layout, c['A'], c['B'], C, adt=dt, bdt=dt, fp8=True, splitk=1)
    assert _only_window_written(buf, C)
    _check_out(f'mx_spread_{layout}_{"bf16" if dt == BF16 else "f32"}', C, ref, True, False, 'plain')


@pytest.mark.parametrize('layout', ['nt', 'nn', 'tn'])
@pytest.mark.parametrize('K,sk', tr.MX_KS)
def test_mx_ragged_k_and_splitk(layout, K, sk):
    """K = 70, 128, 129 (a ragged block, one exact K-tile, one element into the next) and split-K
    2 at K = 300, unaligned A.  Per output row, 1e-4."""
    M, N = tr.RAND_SHAPE[:2]
    c = tr.rand_case(M, N, K)
    ref, _ = tr.gemm_ref(c['A'], c['B'], rounding='mx')
    buf, C = _window(M, N, F32)
    _gemm(layout, c['A'], c['B'], C, fp8=True, splitk=sk, a_aligned=False)
    assert _only_window_written(buf, C)
    _check_out(f'mx_k{K}_sk{sk}_{layout}', C, ref, True, False, 'plain')


# ================================================================ c. act_bwd, dropout_bwd, colsum
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('p', [0.0, tr.P_DROP])
@pytest.mark.parametrize('dydt', [F32, BF16], ids=['dy_f32', 'dy_bf16'])
@pytest.mark.parametrize('odt', [F32, BF16], ids=['out_f32', 'out_bf16'])
def test_act_bwd_vs_float64(act, p, dydt, odt):
    """dy (lddy > N) keep / (1 - p) act'(aux).  f32 output: act 0 / 2 are one rounding, so
    bit-exact, with exact zeros where the mask or the ReLU is off; GELU' within 1e-6 of scale.
    bf16 output: 2^-7."""
    L = _L()
    M, N = tr.ACT_BWD_SHAPE
    c = tr.rand_case(M, N, 8)
    dy = c['C0'].to(dydt)
    aux = (c['resid'] * 1.4).bfloat16()
    mask = _kernel_mask(M, N, p, SEED) if p else None
    ref = tr.act_bwd_ref(dy, aux, act, mask, p)
    dbuf, dview = _window(M, N, dydt)
    dview.copy_(dy)
    obuf, out = _guarded(M * N, odt)
    auxd = aux.to(DEV)
    _call('ewvit_act_bwd', L.ptr(dview), L.dt(dview), dview.stride(0), L.ptr(auxd) if act else None, act, p, SEED,
          None, L.ptr(out), L.dt(out), M, N)
    assert _guard_intact(obuf, M * N)
    got = out.view(M, N).cpu()
    tag = f'act_bwd_act{act}_p{p}'
    if odt == BF16:
        e = tr.err_of_scale(got, ref)
        log(tag + '_bf16', e, tr.BF16_OUT)
        assert e <= tr.BF16_OUT, e
    elif act == 1:
        e = tr.err_of_scale(got, ref)
        log(tag, e, tr.ACT_BWD_GELU)
        assert e <= tr.ACT_BWD_GELU, e
    else:
        assert torch.equal(got, ref.float()), float((got - ref).abs().max())
    off = torch.zeros(M, N, dtype=torch.bool)
    if mask is not None:
        off |= ~mask
    if act == 2:
        off |= ~(aux.float() > 0)
    assert float(got[off].float().abs().max() if off.any() else 0.0) == 0.0


def test_masks_of_forward_and_backward_agree_under_a_device_step_counter():
    """With a device seed_offset, ewvit_act_bwd and ewvit_dropout_bwd regenerate the mask the
    forward GEMM drew (both kernels), another one than without the counter."""
    L = _L()
    M, N = tr.ACT_BWD_SHAPE
    c = tr.rand_case(M, N, 8)
    off = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    base = _kernel_mask(M, N, tr.P_DROP, SEED)
    want = _kernel_mask(M, N, tr.P_DROP, SEED, off)
    assert not torch.equal(base, want)
    for fp8 in (False, True):
        buf, C = _window(M, N, F32)
        _gemm('nt', c['A'], c['B'], C, fp8=fp8, drop_p=tr.P_DROP, seed=SEED, seed_offset=off)
        assert torch.equal(C.cpu() != 0, want)
    ones = torch.ones(M, N, device=DEV)
    out = torch.empty(M, N, device=DEV)
    _call('ewvit_act_bwd', L.ptr(ones), L.F32, N, None, 0, tr.P_DROP, SEED, L.ptr(off), L.ptr(out), L.F32, M, N)
    assert torch.equal(out.cpu() != 0, want)


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_dropout_bwd_strided(dt):
    """g (ldg > cols) *= keep / (1 - p) in place: f32 bit-exact, bf16 within 2^-7; the padding
    stays untouched."""
    L = _L()
    M, N = tr.ACT_BWD_SHAPE
    g0 = tr.rand_case(M, N, 8)['C0'].to(dt)
    mask = _kernel_mask(M, N, tr.P_DROP, SEED)
    ref = tr.act_bwd_ref(g0, None, 0, mask, tr.P_DROP)
    buf, g = _window(M, N, dt)
    g.copy_(g0)
    _call('ewvit_dropout_bwd', L.ptr(g), L.dt(g), M, N, g.stride(0), tr.P_DROP, SEED, None)
    assert _only_window_written(buf, g)
    if dt == F32:
        assert torch.equal(g.cpu(), ref.float())
    else:
        e = tr.err_of_scale(g.cpu(), ref)
        log('dropout_bwd_bf16', e, tr.BF16_OUT)
        assert e <= tr.BF16_OUT and float(g.cpu()[~mask].float().abs().max()) == 0.0


@pytest.mark.parametrize('N', tr.COLSUM_NS)
@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_colsum_strided_accumulate(N, dt):
    """out += column sums of X (ldx > N), N = 1, 64, 65 (one thread, one full block of columns,
    one column into the next): 1e-5 of scale; also overwriting (accumulate = 0)."""
    L = _L()
    M = tr.COLSUM_M
    g = torch.Generator().manual_seed(N)
    X = torch.randn(M, N, generator=g).to(dt)
    o0 = torch.randn(N, generator=g) * 10
    xbuf, Xv = _window(M, N, dt)
    Xv.copy_(X)
    for acc in (1, 0):
        obuf, out = _guarded(N, F32)
        out.copy_(o0)
        _call('ewvit_colsum', L.ptr(Xv), L.dt(Xv), Xv.stride(0), M, N, L.ptr(out), acc)
        assert _guard_intact(obuf, N)
        ref = X.to(F64).sum(0) + (o0.to(F64) if acc else 0)
        e = tr.err_of_scale(out.cpu(), ref)
        log(f'colsum_n{N}_acc{acc}', e, tr.COLSUM)
        assert e <= tr.COLSUM, e


# ================================================================ d. tall-K
@functools.lru_cache(maxsize=None)
def _tallk_dev():
    X, W, b, _ = tr.tallk_case()
    return W.to(DEV), b.to(DEV)


@pytest.mark.parametrize('M', tr.TALLK_MS)
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
def test_tallk_smallest_class_member(M, with_bias):
    """K = 16384, N = 256 (the smallest member of the class), M = 1, 17, 64, lda > K, ldc > N
    inside a NaN buffer: 1e-4 of scale against float64 and against ewvit_gemm with split-K 64."""
    import ewvit
    L = _L()
    K, N = tr.TALLK_K, tr.TALLK_N
    X, _, b, ref = tr.tallk_case()
    Wd, bd = _tallk_dev()
    ref = ref[:M] + (b.to(F64) if with_bias else 0)
    xbuf = torch.full((M, K + 8), NAN, dtype=BF16, device=DEV)
    Xv = xbuf[:, :K]
    Xv.copy_(X[:M])
    nws = int(L.load().ewvit_gemm_tallk_workspace(M, N, K)) // 4
    wbuf, ws = _guarded(nws, F32)
    buf, C = _window(M, N, F32)
    _call('ewvit_gemm_tallk', L.ptr(Xv), Xv.stride(0), L.ptr(Wd), L.ptr(bd) if with_bias else None, L.ptr(C),
          C.stride(0), M, N, K, L.ptr(ws))
    assert _only_window_written(buf, C) and bool(torch.isnan(wbuf[nws:]).all())
    e = tr.err_of_scale(C.cpu(), ref)
    log(f'tallk_m{M}', e, tr.TALLK)
    assert e <= tr.TALLK, e
    buf2, C2 = _window(M, N, F32)
    ewvit.ops.gemm(Xv, (Xv.stride(0), 1), Wd, (1, K), C2, M, N, K, bias=bd if with_bias else None, splitk=64)
    assert _only_window_written(buf2, C2)
    e2 = tr.err_of_scale(C.cpu(), C2.cpu())
    log(f'tallk_vs_gemm_m{M}', e2, tr.TALLK)
    assert e2 <= tr.TALLK and tr.err_of_scale(C2.cpu(), ref) <= tr.TALLK


# ================================================================ e. LayerNorm
def _ln_run(c, xdt=F32, ydt=F32, accumulate=False, grads=True):
    """ewvit_layernorm_fwd + bwd on case c, x with ldx > D inside a NaN buffer, every output and
    the workspace followed by a NaN guard.  -> dict of CPU results."""
    L = _L()
    M, D = c['x'].shape
    xbuf = torch.full((M, D + 3), NAN, dtype=xdt, device=DEV)
    x = xbuf[:, :D]
    x.copy_(c['x'])
    gm, bt, dy = c['gamma'].to(DEV), c['beta'].to(DEV), c['dy'].to(DEV)
    ybuf, y = _guarded(M * D, ydt)
    mbuf, mean = _guarded(M, F32)
    rbuf, rstd = _guarded(M, F32)
    _call('ewvit_layernorm_fwd', L.ptr(x), L.dt(x), x.stride(0), L.ptr(gm), L.ptr(bt), L.ptr(y), L.dt(y), L.ptr(mean),
          L.ptr(rstd), M, D, tr.LN_EPS)
    assert _guard_intact(ybuf, M * D) and _guard_intact(mbuf, M) and _guard_intact(rbuf, M)
    nws = int(L.load().ewvit_layernorm_bwd_workspace(M, D)) // 4
    rpb = 16 if M >= 16384 else 4
    assert nws == (M + rpb - 1) // rpb * 2 * D
    wbuf, ws = _guarded(nws, F32)
    dxbuf, dx = _guarded(M * D, F32)
    if accumulate:
        dx.copy_(c['dx0'].flatten())
    gbuf, dg = _guarded(D, F32)
    bbuf, db = _guarded(D, F32)
    _call('ewvit_layernorm_bwd', L.ptr(dy), L.F32, L.ptr(x), L.dt(x), x.stride(0), L.ptr(gm), L.ptr(mean), L.ptr(rstd),
          L.ptr(dx), int(accumulate), L.ptr(dg) if grads else None, L.ptr(db) if grads else None, L.ptr(ws), M, D)
    assert _guard_intact(dxbuf, M * D) and bool(torch.isnan(wbuf[nws:]).all())
    out = {'y': y.view(M, D).cpu(), 'mean': mean.cpu(), 'rstd': rstd.cpu(), 'dx': dx.view(M, D).cpu()}
    if grads:
        assert _guard_intact(gbuf, D) and _guard_intact(bbuf, D)
        out.update(dgamma=dg.cpu(), dbeta=db.cpu())
    else:
        assert bool(torch.isnan(gbuf).all()) and bool(torch.isnan(bbuf).all())
    return out


def _ln_check(tag, got, c, ybound, bound=tr.LN_F32, accumulate=False):
    worst = {}
    for k, ref in (('y', c['y']), ('mean', c['mean']), ('rstd', c['rstd']),
                   ('dx', c['dx'] + (c['dx0'].to(F64) if accumulate else 0)), ('dgamma', c['dgamma']),
                   ('dbeta', c['dbeta'])):
        if k in got:
            worst[k] = tr.err_of_scale(got[k], ref)
            b = ybound if k == 'y' else bound
            log(f'{tag}_{k}', worst[k], b)
            assert worst[k] <= b, (tag, k, worst[k], b)
    return worst


@pytest.mark.parametrize('xdt', [F32, BF16], ids=['x_f32', 'x_bf16'])
@pytest.mark.parametrize('ydt', [F32, BF16], ids=['y_f32', 'y_bf16'])
def test_layernorm_dtypes_and_lane_edges(xdt, ydt):
    """x f32 / bf16 x y f32 / bf16, ldx > D, D in {1, 63, 64, 65, 1000, 1024} (one lane, the wave
    edge, the register edge) x M in {1, 3, 5} (a partial block of 4 rows, one row into the
    second): 2e-5 of scale in f32 (mean, rstd, dx, dgamma, dbeta as well), 2^-7 for a bf16 y."""
    for D in tr.LN_DS:
        for M in tr.LN_MS:
            c = tr.ln_case(M, D, xdt)
            _ln_check(f'ln_{M}x{D}', _ln_run(c, xdt, ydt), c, tr.BF16_OUT if ydt == BF16 else tr.LN_F32)


def test_layernorm_sixteen_rows_per_block_branch():
    """M = 16384 + 5, D = 96: ln_bwd_rpb's other branch (16 rows per block, its own workspace
    size, a ragged last block).  The workspace is followed by a NaN guard."""
    c = tr.ln_case(*tr.LN_BIG)
    _ln_check('ln_big', _ln_run(c), c, tr.LN_F32)
    L = _L()
    assert int(L.load().ewvit_layernorm_bwd_workspace(16383, 96)) == (16383 + 3) // 4 * 2 * 96 * 4


def test_layernorm_accumulate_dx_and_null_param_grads():
    c = tr.ln_case(5, 65)
    got = _ln_run(c, accumulate=True, grads=False)
    _ln_check('ln_acc', got, c, tr.LN_F32, accumulate=True)
    assert 'dgamma' not in got


def test_layernorm_far_mean_rows():
    """x = 1000 + N(0, 1) held in f32.  Bound: the f32 mean of a row is a tree of additions, each
    rounding by up to 2^-24 |mean|, so mean carries an error of order 2^-23 |mean|; every
    x - mean of the row inherits it and xhat = (x - mean) rstd scales it by 1 / std.  Hence
    2^-23 max|mean| max rstd on xhat (1.2e-4 here), added to the 2e-5 of the near-zero-mean
    case — token_ref.ln_far_bound.  The centred second pass adds nothing of that order; a
    one-pass E[x^2] - mean^2 in f32 loses 2^-24 mean^2 / var ~ 6 % and misses the bound by more
    than 10x (tests/test_token_ref_cpu.py).  Measured on the MI355X: y 1.7e-5 / 2.7e-5, dgamma
    2.7e-5 / 3.7e-5, dx 5.6e-7 / 3.7e-6, dbeta, mean, rstd below 1e-7 (M x D = 5 x 96 / 3 x 1000)."""
    for M, D in ((5, 96), (3, 1000)):
        c = tr.ln_case(M, D, kind='far')
        bound = tr.ln_far_bound(c)
        assert bound < 2e-4
        _ln_check(f'ln_far_{M}x{D}', _ln_run(c), c, bound, bound)


def test_layernorm_constant_rows():
    """Rows of one value (0, 1, -2.5, 3.7, 1000.1): variance 0, rstd = eps^-1/2 = 316.  y = beta,
    every output finite.  dx is rstd (g - mean g), g = dy gamma — NOT zero for a general dy (float64
    autograd of F.layer_norm agrees, tests/test_token_ref_cpu.py); it is zero when g is constant
    along the row, which is checked with dy = 1 / gamma.  Bound per row: the far-mean bound with
    std = sqrt(eps) and the worst case of the mean's 8 roundings, 2e-5 + 8 2^-24 |value| 316 (a row
    whose f32 sum is exact gives exactly beta).  Measured: 0.13 of it on y, 3e-3 of it on dx."""
    M, D = 5, 96
    c = tr.ln_case(M, D, kind='const')
    got = _ln_run(c)
    vals = c['x'][:, 0].to(F64).abs()
    rs = float(c['rstd'].max())
    # the error of xhat, per row: here the roundings of the sum's (D / 64 serial + 6 tree) additions and
    # of the division do not average out over a row of equal values, so the worst case 2^-24 each
    slack = ((D + 63) // 64 + 6) * 2.0 ** -24 * vals * rs
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), k
    gmax = float(c['gamma'].abs().max())
    ey = (got['y'].to(F64) - c['beta'].to(F64)).abs().amax(1)
    by = tr.LN_F32 * float(c['beta'].abs().max()) + slack * gmax
    log('ln_const_y', float((ey / by).max()), 1.0)
    assert bool((ey <= by).all()), (ey, by)
    assert torch.equal(got['y'][:3], c['beta'].expand(3, D))        # 0, 1, -2.5: exact sums
    g = (c['dy'] * c['gamma']).to(F64)
    edx = (got['dx'].to(F64) - c['dx']).abs().amax(1)
    bdx = (tr.LN_F32 + slack) * c['dx'].abs().amax(1)
    log('ln_const_dx', float((edx / bdx).max()), 1.0)
    assert bool((edx <= bdx).all()), (edx, bdx)
    assert float(got['dgamma'].abs().max()) <= float(c['dy'].abs().max()) * float(slack.sum()) + 1e-30
    assert tr.err_of_scale(got['dbeta'], c['dbeta']) <= tr.LN_F32
    # dy gamma constant along each row: dx = 0
    flat = dict(c)
    flat['dy'] = (1.0 / c['gamma']).expand(M, D).contiguous()
    dx0 = _ln_run(flat)['dx'].to(F64).abs().amax(1)
    b0 = (tr.LN_F32 + slack) * rs
    log('ln_const_dx_flat', float((dx0 / b0).max()), 1.0)
    assert bool((dx0 <= b0).all()), (dx0, b0)


# ================================================================ f. attention
def _strided(t, pad=8):
    """t [B, n, W] as a slice of a NaN-filled [B, n + 1, W + pad] buffer."""
    B, n, W = t.shape
    buf = torch.full((B, n + 1, W + pad), NAN, dtype=t.dtype, device=DEV)
    v = buf[:, :n, :W]
    v.copy_(t)
    return buf, v


def _pad_is_nan(buf, n, W):
    return bool(torch.isnan(buf[:, n:]).all()) and bool(torch.isnan(buf[:, :, W:]).all()) and \
        bool(torch.isfinite(buf[:, :n, :W]).all())


def _attn_run(c, packed, H, d):
    """ewvit_attn_fwd + bwd with q / k / v / do / o and the gradients as strided slices of wider
    NaN-filled buffers (packed: one qkv buffer, one gradient buffer).  -> CPU results."""
    L = _L()
    B, nq, inner = c['q'].shape
    nk = c['k'].shape[1]
    if packed:
        sbuf, src = _strided(torch.cat([c['q'], c['k'], c['v']], -1))
        q, k, v = src[..., :inner], src[..., inner:2 * inner], src[..., 2 * inner:]
        gbuf = torch.full_like(sbuf, NAN)
        g = gbuf[:, :nq, :3 * inner]
        dq, dk, dv = g[..., :inner], g[..., inner:2 * inner], g[..., 2 * inner:]
    else:
        qbuf, q = _strided(c['q'])
        kvbuf, kv = _strided(torch.cat([c['k'], c['v']], -1))
        k, v = kv[..., :inner], kv[..., inner:]
        dqbuf, dkvbuf = torch.full_like(qbuf, NAN), torch.full_like(kvbuf, NAN)
        dq = dqbuf[:, :nq, :inner]
        dk, dv = dkvbuf[:, :nk, :inner], dkvbuf[:, :nk, inner:2 * inner]
    obuf = torch.full((B, nq + 1, inner + 8), NAN, dtype=BF16, device=DEV)
    o = obuf[:, :nq, :inner]
    pbuf, p = _guarded(B * H * nq * nk, F32)
    _call('ewvit_attn_fwd', L.ptr(q), q.stride(0), q.stride(1), L.ptr(k), k.stride(0), k.stride(1), L.ptr(v),
          v.stride(0), v.stride(1), L.ptr(o), o.stride(0), o.stride(1), L.ptr(p), B, H, nq, nk, d, c['scale'])
    assert _pad_is_nan(obuf, nq, inner) and _guard_intact(pbuf, p.numel())
    dobuf, do = _strided(c['do'])
    _call('ewvit_attn_bwd', L.ptr(do), do.stride(0), do.stride(1), L.ptr(q), q.stride(0), q.stride(1), L.ptr(k),
          k.stride(0), k.stride(1), L.ptr(v), v.stride(0), v.stride(1), L.ptr(p), L.ptr(dq), L.ptr(dk), L.ptr(dv),
          B, H, nq, nk, d, c['scale'])
    if packed:
        assert _pad_is_nan(gbuf, nq, 3 * inner)
    else:
        assert _pad_is_nan(dqbuf, nq, inner) and _pad_is_nan(dkvbuf, nk, 2 * inner)
    return {'o': o.cpu(), 'p': p.view(B, H, nq, nk).cpu(), 'dq': dq.cpu(), 'dk': dk.cpu(), 'dv': dv.cpu()}


def _attn_check(tag, got, c, check_p=True):
    worst = {}
    for k, b in (('o', tr.ATTN_FWD), ('dq', tr.ATTN_GRAD), ('dk', tr.ATTN_GRAD), ('dv', tr.ATTN_GRAD)):
        worst[k] = tr.err_of_scale(got[k], c[k])
        log(f'{tag}_{k}', worst[k], b)
        assert worst[k] <= b, (tag, k, worst[k], b)
    psum = float((got['p'].to(F64).sum(-1) - 1).abs().max())
    log(f'{tag}_psum', psum, tr.ATTN_P_SUM)
    assert psum <= tr.ATTN_P_SUM, (tag, psum)
    if check_p:
        pe = float((got['p'].to(F64) - c['p']).abs().max())
        log(f'{tag}_p', pe, tr.ATTN_P)
        assert pe <= tr.ATTN_P, (tag, pe)
    return worst


@pytest.mark.parametrize('packed', [False, True], ids=['cross', 'packed'])
@pytest.mark.parametrize('B,H', tr.ATTN_BH)
def test_attention_every_sequence_length(packed, B, H):
    """Every (nq, nk) in 1..8 x 1..8 at d = 32 (packed: nq = nk), B H = 1, 5, 21 (one wave, a
    partial block of 4 waves, several blocks): outputs 1e-2, gradients 1.5e-2 of scale (bf16 I/O);
    the saved p sums to 1 within 1e-6 per row and equals the float64 softmax within 1e-5."""
    d = tr.ATTN_D_SWEEP
    for nq in range(1, 9):
        for nk in ((nq,) if packed else range(1, 9)):
            c = tr.attn_case(packed, B, H, nq, nk, d)
            _attn_check(f'attn_{"p" if packed else "c"}_{nq}x{nk}', _attn_run(c, packed, H, d), c)


@pytest.mark.parametrize('d', tr.ATTN_DS)
def test_attention_head_dim_edges(d):
    """d = 1, 63, 64, 65, 127, 128 (64: the second element per lane begins) at 2 x 2 packed and
    cross and at 1 x 2 cross."""
    B, H = 7, 3
    for packed, nq, nk in ((True, 2, 2), (False, 2, 2), (False, 1, 2)):
        c = tr.attn_case(packed, B, H, nq, nk, d)
        _attn_check(f'attn_d{d}_{nq}x{nk}', _attn_run(c, packed, H, d), c)


@pytest.mark.parametrize('packed,B,H,nq,nk', tr.ATTN_BIG)
def test_attention_logits_of_order_hundred(packed, B, H, nq, nk):
    """q and k scaled so the logits reach +-100: outputs and gradients finite and inside the same
    bounds against float64 on the same bf16 inputs; rows whose float64 softmax is one-hot in f32
    (both forms have some, tests/test_token_ref_cpu.py) are one-hot in the saved p: 1 exactly,
    the rest below 2^-100."""
    d = tr.ATTN_D_SWEEP
    c = tr.attn_case(packed, B, H, nq, nk, d, big=True)
    assert float(c['logits'].abs().max()) >= 100
    got = _attn_run(c, packed, H, d)
    for k in got:
        assert bool(torch.isfinite(got[k].float()).all()), k
    _attn_check(f'attn_big_{"p" if packed else "c"}_{nq}x{nk}', got, c, check_p=False)
    hot = tr.one_hot_rows(c['p'])
    log(f'attn_big_{"p" if packed else "c"}_{nq}x{nk}_one_hot_rows', int(hot.sum()), hot.numel())
    if bool(hot.any()):
        ph, rh = got['p'][hot], c['p'][hot]
        assert torch.equal(ph.argmax(-1), rh.argmax(-1))
        assert torch.equal(ph.amax(-1), torch.ones(ph.shape[0]))
        assert float((ph * (ph < 1)).to(F64).sum(-1).max()) <= 2.0 ** -100


# ================================================================ g. refusals
def test_bad_arguments_are_refused_before_any_launch():
    """Each call must raise with the library's message and leave its output untouched."""
    import ewvit
    L = _L()
    A, B = torch.randn(8, 32, device=DEV), torch.randn(16, 32, device=DEV)

    def gemm(C, **kw):
        ewvit.ops.gemm(A, kw.pop('lda', (32, 1)), B, (1, 32), C, 8, 16, 32, **kw)

    Cb = torch.full((8, 16), NAN, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match='beta needs f32 C'):
        gemm(Cb, beta=1.0)
    assert bool(torch.isnan(Cb).all())
    C = torch.full((8, 16), NAN, device=DEV)
    with pytest.raises(RuntimeError, match='act 3 needs aux'):
        gemm(C, act=3)
    with pytest.raises(RuntimeError, match='A needs a unit stride'):
        gemm(C, lda=(64, 2))
    with pytest.raises(RuntimeError, match='split-K needs a workspace'):
        _call('ewvit_gemm', L.ptr(A), L.F32, 32, 1, L.ptr(B), L.F32, 1, 32, L.ptr(C), L.F32, 16, 8, 16, 32, 1.0, 0.0,
              None, 0, None, 0.0, 0, None, None, 0, 0, 2, None)
    with pytest.raises(RuntimeError, match='split-K needs a workspace'):
        _call('ewvit_gemm_mx8', L.ptr(A), L.F32, 32, 1, L.ptr(B), L.F32, 1, 32, L.ptr(C), L.F32, 16, 8, 16, 32, 1.0,
              0.0, None, 0, None, 0.0, 0, None, None, 0, 0, 2, None)
    assert bool(torch.isnan(C).all())
    # LayerNorm D = 1025
    D = 1025
    x, gm = torch.randn(2, D, device=DEV), torch.ones(D, device=DEV)
    y = torch.full((2, D), NAN, device=DEV)
    st = torch.full((2,), NAN, device=DEV)
    with pytest.raises(RuntimeError, match=r'layernorm_fwd: D=1025 not in \(0,1024\]'):
        _call('ewvit_layernorm_fwd', L.ptr(x), L.F32, D, L.ptr(gm), L.ptr(gm), L.ptr(y), L.F32, L.ptr(st), L.ptr(st),
              2, D, 1e-5)
    with pytest.raises(RuntimeError, match=r'layernorm_bwd: D=1025 not in \(0,1024\]'):
        _call('ewvit_layernorm_bwd', L.ptr(x), L.F32, L.ptr(x), L.F32, D, L.ptr(gm), L.ptr(st), L.ptr(st), L.ptr(y), 0,
              None, None, L.ptr(y), 2, D)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(st).all())
    # attention nk = 9, d = 129
    t = torch.zeros(2, 9, 2 * 129, dtype=BF16, device=DEV)
    o = torch.full((2, 9, 129), NAN, dtype=BF16, device=DEV)
    p = torch.full((2 * 9 * 9,), NAN, device=DEV)
    for nk, d, msg in ((9, 32, r'attn_fwd: nq=1 nk=9 outside \[1,8\]'), (2, 129, r'attn_fwd: head dim 129 outside \[1,128\]')):
        with pytest.raises(RuntimeError, match=msg):
            _call('ewvit_attn_fwd', L.ptr(t), t.stride(0), t.stride(1), L.ptr(t), t.stride(0), t.stride(1), L.ptr(t),
                  t.stride(0), t.stride(1), L.ptr(o), o.stride(0), o.stride(1), L.ptr(p), 2, 1, 1, nk, d, 1.0)
        with pytest.raises(RuntimeError, match=msg.replace('attn_fwd', 'attn_bwd')):
            _call('ewvit_attn_bwd', L.ptr(t), t.stride(0), t.stride(1), L.ptr(t), t.stride(0), t.stride(1), L.ptr(t),
                  t.stride(0), t.stride(1), L.ptr(t), t.stride(0), t.stride(1), L.ptr(p), L.ptr(o), L.ptr(o), L.ptr(o),
                  2, 1, 1, nk, d, 1.0)
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(p).all())
    # tall-K with N = 128
    X = torch.zeros(4, 16384, dtype=BF16, device=DEV)
    W = torch.zeros(128, 16384, device=DEV)
    Ct = torch.full((4, 128), NAN, device=DEV)
    ws = torch.full((64 * 64 * 128,), NAN, device=DEV)
    with pytest.raises(RuntimeError, match='gemm_tallk: M=4 N=128 K=16384 outside its shape class'):
        _call('ewvit_gemm_tallk', L.ptr(X), 16384, L.ptr(W), None, L.ptr(Ct), 128, 4, 128, 16384, L.ptr(ws))
    assert bool(torch.isnan(Ct).all()) and bool(torch.isnan(ws).all())
    # and mm_nt does not route that shape to it
    assert not ewvit.ops._tallk(X, W, Ct, {})

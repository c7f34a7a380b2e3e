"""The float64 references of tests/token_ref.py checked on the CPU, independently of the kernels
they are the yardstick for (tests/test_gpu_token_ops.py).

* `gemm_ref` equals the torch float64 composition F.linear -> GELU / ReLU -> mask -> + residual
  (-> + beta C0) on the rounded operands, its act 3 and `act_bwd_ref` equal float64 autograd of
  that composition; the LayerNorm and attention references equal F.layer_norm / softmax attention
  under float64 autograd.
* Every bound of the GPU file rejects a deliberately wrong result built from the GPU file's own
  inputs: one K element dropped from one output row at the longest K, one MX block scaled 2x in
  each of NT, NN and TN, the dropout mask shifted by one column, the residual added before the
  dropout, a one-pass f32 LayerNorm variance on the far-mean rows (missed by more than 10x), one
  key left out of a softmax.
* Every cap the GPU file asserts holds for the reference's own data: exact-integer sums below
  2^24, at most 0.1 % of the ReLU outputs left out, logits that do reach +-100 with one-hot rows
  among them, no operand above about 2 M elements but the tall-K weight the issue's smallest
  class member needs.
"""
import pytest
import torch
import torch.nn.functional as F

import token_ref as tr

F64 = torch.float64


def _mask_for(c):
    return c['cpu_mask']


# ---------------------------------------------------------------- references against torch
@pytest.mark.parametrize('rounding', ['bf16', 'mx'])
@pytest.mark.parametrize('act', [0, 1, 2])
def test_gemm_ref_equals_torch_composition(rounding, act):
    M, N, K = tr.RAND_SHAPE
    c = tr.rand_case(M, N, K)
    rnd = tr.bf16 if rounding == 'bf16' else tr.mxq
    x = rnd(c['A'])                                   # [M, K]
    w = rnd(c['B'].t())                               # [N, K]: nn.Linear's weight, blocks along K
    m = _mask_for(c).to(F64) * tr.drop_scale(tr.P_DROP)
    pre = 0.5 * F.linear(x, w) + c['bias'].to(F64)
    h = F.gelu(pre) if act == 1 else torch.relu(pre) if act == 2 else pre
    want = h * m + c['resid'].to(F64) + 0.5 * c['C0'].to(F64)
    y, p = tr.gemm_ref(c['A'], c['B'], rounding=rounding, alpha=0.5, beta=0.5, C0=c['C0'], bias=c['bias'], act=act,
                       mask=_mask_for(c), p=tr.P_DROP, resid=c['resid'])
    assert tr.err_of_scale(y, want) < 1e-14
    assert tr.err_of_scale(p, pre) < 1e-14


def test_act3_and_act_bwd_ref_equal_autograd():
    M, N, K = tr.RAND_SHAPE
    c = tr.rand_case(M, N, K)
    aux = (c['resid'] * 1.4).bfloat16()
    h = aux.to(F64).requires_grad_(True)
    F.gelu(h).sum().backward()
    y3, _ = tr.gemm_ref(c['A'], c['B'], act=3, aux=aux)
    assert tr.err_of_scale(y3, (tr.bf16(c['A']) @ tr.bf16(c['B'])) * h.grad) < 1e-14
    dy, mask = c['C0'], _mask_for(c)
    for act in (0, 1, 2):
        h = aux.to(F64).requires_grad_(True)
        a = F.gelu(h) if act == 1 else torch.relu(h) if act == 2 else h
        (a * mask.to(F64) * tr.drop_scale(tr.P_DROP) * dy.to(F64)).sum().backward()
        assert tr.err_of_scale(tr.act_bwd_ref(dy, aux, act, mask, tr.P_DROP), h.grad) < 1e-14
    assert torch.equal(tr.act_bwd_ref(dy, aux, 0, None, 0.0), dy.to(F64))


@pytest.mark.parametrize('kind', ['rand', 'far', 'const'])
def test_layernorm_refs_equal_torch_autograd(kind):
    c = tr.ln_case(5, 96, kind=kind)
    x, g, b = (c[k].to(F64).requires_grad_(True) for k in ('x', 'gamma', 'beta'))
    y = F.layer_norm(x, (96,), g, b, tr.LN_EPS)
    y.backward(c['dy'].to(F64))
    assert tr.err_of_scale(c['y'], y) < 1e-12
    for got, want in ((c['dx'], x.grad), (c['dgamma'], g.grad), (c['dbeta'], b.grad)):
        d = float((got - want).abs().max())
        assert d <= 1e-9 * max(float(want.abs().max()), 1.0), d      # a constant row's xhat: 1e-13 * rstd 316
    if kind == 'const':
        # variance 0: y is beta, dgamma 0; dx = rstd (g - mean g) is NOT zero unless dy gamma is constant on the row
        assert torch.equal(c['y'], c['beta'].to(F64).expand(5, 96))
        assert float(c['dgamma'].abs().max()) == 0.0 and float(c['dx'].abs().max()) > 1.0
        flat = (torch.ones(5, 96, dtype=F64) / c['gamma'].to(F64))
        assert float(tr.layernorm_bwd_ref(flat, c['x'].to(F64), c['mean'], c['rstd'], c['gamma'].to(F64))[0].abs().max()) < 1e-10


@pytest.mark.parametrize('nq,nk,d', [(1, 2, 32), (2, 2, 64), (8, 8, 32), (3, 8, 65)])
def test_attention_refs_equal_torch_autograd(nq, nk, d):
    B, H = 5, 3
    c = tr.attn_case(False, B, H, nq, nk, d)
    q, k, v = (tr.heads_of(c[n], H, d).to(F64).requires_grad_(True) for n in ('q', 'k', 'v'))
    o = torch.softmax(q @ k.transpose(-1, -2) * c['scale'], -1) @ v
    o.backward(tr.heads_of(c['do'], H, d).to(F64))
    assert tr.err_of_scale(c['o'], tr.tokens_of(o)) < 1e-13
    for n, t in (('dq', q), ('dk', k), ('dv', v)):
        assert tr.err_of_scale(c[n], tr.tokens_of(t.grad)) < 1e-12
    assert float((c['p'].sum(-1) - 1).abs().max()) < 1e-14
    if d == 64:
        want = F.scaled_dot_product_attention(q, k, v)
        assert tr.err_of_scale(c['o'], tr.tokens_of(want)) < 1e-13


def test_place_keeps_values_and_strides():
    X = torch.arange(15.0).reshape(3, 5)
    for kc in (True, False):
        for al in (True, False):
            v, s = tr.place(X, kc, torch.float32, al)
            assert torch.equal(v, X) and v.stride() == s
            assert (s[0] if kc else s[1]) % 8 == (0 if al else 3)


# ---------------------------------------------------------------- the checks bite
def test_bites_dropped_k_element_at_longest_k():
    K = max(k for k, _ in tr.INT_K)
    A, B = tr.int_operands()
    A, B = A[:130, :K].clone(), B[:K, :130]
    ref = tr.int_ref(130, 130, K)
    k = next(i for i in range(K // 2, K) if A[7, i] != 0)
    A[7, k] = 0
    wrong = A @ B
    assert not torch.equal(wrong.float(), ref.float())              # the exact-integer check
    assert torch.equal(wrong[:7], ref[:7]) and torch.equal(wrong[8:], ref[8:])
    # and the random-data bounds at their longest K
    for rounding, bound, per_row, (M, N, Kr) in (('bf16', tr.GEMM_PLAIN, False, tr.RAND_SHAPE),
                                                 ('mx', tr.MX_ROW, True, (70, 93, max(k for k, _ in tr.MX_KS)))):
        c = tr.rand_case(M, N, Kr)
        ref, _ = tr.gemm_ref(c['A'], c['B'], rounding=rounding)
        A2 = c['A'].clone()
        A2[7, Kr // 2] = 0
        assert tr.err_of_scale(tr.gemm_ref(A2, c['B'], rounding=rounding)[0], ref, per_row) > 10 * bound


@pytest.mark.parametrize('layout', ['nt', 'nn', 'tn'])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
def test_bites_one_mx_block_scaled_twice(layout, dt):
    """The block is taken from the operand that layout quantizes out of its LDS image (B for NN, A
    for TN; A's register path for NT), in the last, ragged K-tile."""
    M, N, K = tr.MX_SPREAD_SHAPE
    c = tr.rand_case(M, N, K, spread=6, adt=dt, bdt=dt)
    ref, _ = tr.gemm_ref(c['A'], c['B'], rounding='mx')
    qa, qb = tr.mxq(c['A']), tr.mxq(c['B'].t()).t()
    blk = slice(K - 32, K)
    if layout == 'nn':
        qb = qb.clone()
        qb[blk, 11] *= 2
    else:
        qa = qa.clone()
        qa[5, blk] *= 2
    err = tr.err_of_scale(qa @ qb, ref, per_row=True)
    assert err > 10 * tr.MX_ROW, err


def test_bites_mask_shift_and_residual_order():
    M, N, K = tr.RAND_SHAPE
    c = tr.rand_case(M, N, K)
    mask = _mask_for(c)
    kw = dict(bias=c['bias'], act=1, p=tr.P_DROP, resid=c['resid'])
    for rounding, per_row in (('bf16', False), ('mx', True)):
        ref, _ = tr.gemm_ref(c['A'], c['B'], rounding=rounding, mask=mask, **kw)
        shifted, _ = tr.gemm_ref(c['A'], c['B'], rounding=rounding, mask=torch.roll(mask, 1, 1), **kw)
        assert tr.err_of_scale(shifted, ref, per_row) > 100 * tr.GEMM_EPI
        h, _ = tr.gemm_ref(c['A'], c['B'], rounding=rounding, bias=c['bias'], act=1)
        before = (h + c['resid'].to(F64)) * mask.to(F64) * tr.drop_scale(tr.P_DROP)
        assert tr.err_of_scale(before, ref, per_row) > 100 * tr.GEMM_EPI
    # act_bwd: the same shift against its bit-exact / 1e-6 / 2^-7 bounds
    Ma, Na = tr.ACT_BWD_SHAPE
    ca = tr.rand_case(Ma, Na, 8)
    aux = ca['resid'].bfloat16()
    for act in (0, 1, 2):
        ref = tr.act_bwd_ref(ca['C0'], aux, act, ca['cpu_mask'], tr.P_DROP)
        bad = tr.act_bwd_ref(ca['C0'], aux, act, torch.roll(ca['cpu_mask'], 1, 1), tr.P_DROP)
        assert tr.err_of_scale(bad, ref) > 10 * tr.BF16_OUT


def test_bites_one_pass_variance_on_far_mean_rows():
    M, D = 5, 96
    c = tr.ln_case(M, D, kind='far')
    bound = tr.ln_far_bound(c)
    assert tr.LN_F32 < bound < 2e-4                      # 2e-5 + 2^-23 * ~1000 / ~1
    bad = tr.ln_onepass_f32(c['x'], c['gamma'], c['beta'], tr.LN_EPS)
    assert tr.err_of_scale(bad, c['y']) > 10 * bound
    # the two-pass form in f32 (what the kernel does, in torch) is inside it
    good = F.layer_norm(c['x'], (D,), c['gamma'], c['beta'], tr.LN_EPS)
    assert tr.err_of_scale(good, c['y']) < bound


def test_bites_one_key_left_out():
    B, H, nq, nk, d = 5, 1, 8, 8, tr.ATTN_D_SWEEP
    c = tr.attn_case(False, B, H, nq, nk, d)
    q, k, v, do = (tr.heads_of(c[n], H, d) for n in ('q', 'k', 'v', 'do'))
    o, p = tr.attn_ref(q, k[:, :, :-1], v[:, :, :-1], c['scale'])
    assert tr.err_of_scale(tr.tokens_of(o), c['o']) > 3 * tr.ATTN_FWD
    assert float((p - c['p'][..., :-1]).abs().max()) > 100 * tr.ATTN_P
    dq, dk, dv = tr.attn_bwd_ref(do, q, k[:, :, :-1], v[:, :, :-1], p, c['scale'])
    assert tr.err_of_scale(tr.tokens_of(dq), c['dq']) > 3 * tr.ATTN_GRAD
    assert tr.err_of_scale(tr.tokens_of(dk), c['dk'][:, :-1]) > 3 * tr.ATTN_GRAD


# ---------------------------------------------------------------- the caps hold for the reference
def test_caps_exact_integer_sums():
    A, B = tr.int_operands()
    assert float(A.abs().max()) == 8 and float(B.abs().max()) == 8
    assert float((A.abs() @ B.abs()).max()) < 2 ** 24
    assert torch.equal(A.bfloat16().to(F64), A) and torch.equal(B.bfloat16().to(F64), B)
    for M in tr.INT_M:
        for K, _ in tr.INT_K:
            r = tr.int_ref(M, 130, K)
            assert torch.equal(r.float().to(F64), r)


@pytest.mark.parametrize('rounding', ['bf16', 'mx'])
def test_caps_relu_left_out(rounding):
    M, N, K = tr.RAND_SHAPE
    c = tr.rand_case(M, N, K)
    _, pre = tr.gemm_ref(c['A'], c['B'], rounding=rounding, bias=c['bias'], act=2)
    keep, out = tr.relu_keep(pre)
    assert out <= tr.RELU_CAP and bool(keep.any())


def test_caps_sizes_and_attention_logits():
    M, N, K = tr.RAND_SHAPE
    assert max(M * K, K * N, M * N) <= 2_000_000 and 130 * 4096 <= 2_000_000
    assert tr.LN_BIG[0] * tr.LN_BIG[1] <= 2_000_000 and tr.LN_BIG[0] >= 16384
    assert tr.TALLK_K >= 16384 and tr.TALLK_K % 256 == 0 and tr.TALLK_N == 256      # the smallest class member
    hot_rows = {False: 0, True: 0}
    for packed, B, H, nq, nk in tr.ATTN_BIG:
        c = tr.attn_case(packed, B, H, nq, nk, tr.ATTN_D_SWEEP, big=True)
        assert float(c['logits'].abs().max()) >= 100
        hot = tr.one_hot_rows(c['p'])
        hot_rows[packed] += int(hot.sum())
        assert int(hot.sum()) < hot.numel() // 2         # mostly live rows:
        for n in ('dq', 'dk', 'dv'):
            assert float(c[n].abs().max()) > 1           # ... they set the gradients' scale
    assert hot_rows[False] > 0 and hot_rows[True] > 0    # saturated rows in both forms
    # every block of the spread operands has its own scale: the E8M0 exponents of a row differ
    Ms, Ns, Ks = tr.MX_SPREAD_SHAPE
    s = tr.rand_case(Ms, Ns, Ks, spread=6)
    amax = s['A'].abs().view(Ms, Ks // 32, 32).amax(-1)
    assert float((amax.log2().floor().amax(1) - amax.log2().floor().amin(1)).min()) >= 1

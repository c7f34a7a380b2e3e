"""The fused DAMA frame head (csrc/head.hip) checked stage by stage against float64, with the
reference's dropout (p = 0.1 after every to_out and inside gate_net) ON.

ewvit_head_fwd / ewvit_head_bwd leave every intermediate in their fp32 workspace (`struct HeadWs`).
Each stage is recomputed in float64 (tests/fused_ref.py, proven against the oracle on the CPU in
tests/test_fused_ref_cpu.py) FROM THE KERNEL'S OWN STORED INPUTS to that stage, with the operand
rounding the kernel applies there (bf16, or MXFP8 blocks for the attention blocks' GEMMs when
mx=True), so only fp32 accumulation order separates the two sides and stage errors do not
compound.  Bound: max |err| <= 1e-4 of the buffer's max |ref| — the project's bound for an
fp32-accumulated product against a float64 emulation of the same rounded operands
(test_fp8_gemm_vs_torch_e4m3_emulation).  Every measured value is logged next to the bound under
EWVIT_PARITY_LOG.

Stage boundaries, as the kernels round (read off csrc/head.hip):
* every GEMM operand is rounded from the fp32 value that is also stored (xn, the states, o, dpre,
  dq, dkv, dy, dh1), so each stored buffer is a clean boundary;
* the MX forms quantize their activation operands from the bf16 LDS copy of those values, their
  weights and the weight-gradient operands from fp32; the fusion conv's centre tap and the gate's
  first layer stay bf16 in both forms;
* d(attention output) = dpre Wo and the two streams' running gradients are not stored: dq / dkv are
  checked from dpre through to_out's input gradient and the attention backward, and dpre, ds0, df0
  from the streams rebuilt out of the stored buffers (fused_ref._head_streams).

The dropout masks are never generated here: the to_out masks (sites 0-3) are recovered from the
forward (an element was kept iff st[xout] != st[xin]), the gate mask (site 4) from the backward
(dh1 / (dz2 W2) on ReLU-live units).  With them injected the stage checks show that forward,
backward and weight-gradient kernels used one mask; the masks' statistics, their dependence on
the site, the GLOBAL frame and the step counter are asserted directly.  An element equal in both
states whose pre-dropout value is below 1e-4 of scale cannot be read (it is counted as kept) and
is left out of that site's dpre comparison; a live gate unit
with |dz2 W2| below 1e-4 of scale is settled from the forward's softmax weights instead.

Measured (MI355X): bf16 stages 3e-8 .. 3e-7 of scale.  MXFP8 stages 1e-5 .. 8e-5: the scaled
MFMA's own accumulation is coarser than an fp32 sum (about 2^-12 of a dot product's largest
term; ewvit_gemm_mx8's pinned emulation test sits at 1.2e-5 .. 4.2e-5 for the same reason).  The
MX weight gradients reduce over at most 64 frames, so one large term weighs most there: 5e-5 ..
8.1e-5 with the step counter pinned as below, and 1.4e-4 on to_q's gradient of block 2 at N = 64
in a run with whatever counter the process had reached (other masks).  The bound is not
widened for it; the counter is pinned so that every figure is reproducible.

The end-to-end anchor (bf16) compares the whole head with the float64 oracle modules carrying
the recovered masks in place of their Dropouts, at the project's oracle bounds; with another
step's masks the same comparison must fail.
"""
import copy
import functools

import pytest
import torch

import fused_ref as fr
from test_gpu_modules import cos, log

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F64 = torch.float64
BOUND = 1e-4
P_DROP = 0.1
NS = [64, 37, 17, 5]          # 37: two full 16-frame groups + a 5-row tail; 17: a 1-row tail; 5: one partial group


@functools.lru_cache(maxsize=None)
def _base(training):
    from test_gpu_head import _dama
    return _dama(training)


def _model(training, p):
    m = copy.deepcopy(_base(training))
    for layer in m.cross_att.layers:
        layer[1].to_out[1].p = p
        layer[3].to_out[1].p = p
    m.gate_net[4].p = p
    return m


@functools.lru_cache(maxsize=None)
def _run(N, mx, training=True, p=P_DROP, step=0):
    """One forward + backward of the fused head; everything it wrote, on the CPU in float64:
    (cfg with the recovered masks, buffers by name, recovery bookkeeping)."""
    import ewvit
    from ewvit import head as eh
    m = _model(training, p)
    ts = eh.params_of(m)
    bn = m.fusion_gate[1]
    bn0 = (bn.running_mean.detach().to('cpu', F64), bn.running_var.detach().to('cpu', F64),
           int(bn.num_batches_tracked), bn.momentum, bn.eps)
    s0c, f0c, gs = fr.head_inputs(N)
    s0, f0 = s0c.to(DEV).requires_grad_(True), f0c.to(DEV).requires_grad_(True)
    # the device step counter from a fixed start, so the masks (and every figure below) do not
    # depend on what ran earlier in the process: step k is k + 1 advances past zero
    ewvit._lib.rng_offset(s0.device).zero_()
    for _ in range(step + 1):
        ewvit._lib.rng_advance(s0.device)
    fused, s, f = eh.dama_head(m, s0, f0, 12345 + step, mx=mx)
    ws = fused.grad_fn.saved_tensors[0]
    nbytes = int(ewvit._lib.load().ewvit_head_workspace())
    torch.cuda.synchronize()
    fwd = fr.head_ws_views(ws.detach().cpu().clone(), nbytes, N)
    torch.autograd.backward([fused, s, f], [g.to(DEV) for g in gs])
    torch.cuda.synchronize()
    bwd = fr.head_ws_views(ws.detach().cpu().clone(), nbytes, N)
    lay, _ = fr.head_layout()
    first_bwd = next(k for k, (name, _, _) in enumerate(lay) if name == 'dxn0')
    b = {}
    for k, (name, _, _) in enumerate(lay):
        if k < first_bwd:       # the backward leaves what the forward stored alone
            assert torch.equal(fwd[name], bwd[name]), name
        b[name] = (fwd if k < first_bwd else bwd)[name].to(F64)
    b.update({'g_fused': gs[0].to(F64), 'g_s': gs[1].to(F64), 'g_f': gs[2].to(F64),
              'fused': fused.detach().to('cpu', F64), 's_out': s.detach().to('cpu', F64),
              'f_out': f.detach().to('cpu', F64), 'ds0': s0.grad.to('cpu', F64), 'df0': f0.grad.to('cpu', F64),
              'bn_rm': bn.running_mean.detach().to('cpu', F64), 'bn_rv': bn.running_var.detach().to('cpu', F64),
              'bn_nbt': int(bn.num_batches_tracked)})
    for name, t in zip(fr.HEAD_PARAM_NAMES, ts):
        assert t.grad is not None, name
        b['g.' + name] = t.grad.detach().to('cpu', F64)
    P = fr.head_params(ts)
    rounding = 'mx' if mx else 'bf16'
    pe = p if training else 0.0
    masks, info = {}, {}
    for i in range(4):
        pre = fr.linear(b[f'o{i}'], P[f'ca{i}.wo'], rounding) + P[f'ca{i}.bo']
        masks[i], kept, unreadable, small = fr.recover_ca_mask(fwd[f'st{fr.h_xin(i)}'], fwd[f'st{fr.h_xout(i)}'],
                                                               pre, pe)
        info[i] = {'kept': kept, 'unreadable': unreadable, 'small': small}
    m4, kept, live, unreadable, ok = fr.recover_gate_mask(b['dh1'], b['dz2'], b['h1'], P['g1b'], P['g2w'], pe)
    masks[4] = fr.resolve_gate_unreadable(m4, unreadable, b['h1'], P['g1b'], P['g2w'], P['g2b'], b['gw'], pe)
    info[4] = {'kept': masks[4] > 0, 'live': live, 'unreadable': unreadable, 'ok': ok}
    c = fr.HeadCfg(P, masks, rounding, training, bn0, m.cross_att.layers[0][0].eps)
    return c, b, info


def _check_pairs(tag, stages, c, b, info):
    bad = []
    n = 0
    for stage, name, got, ref in fr.stage_pairs(stages, b):
        if name == 'g.bfg' and c.training:
            # a bias feeding a train-mode BatchNorm has a zero true gradient: rounding noise only
            err, bound = float(got.abs().max()) / float(b['g.wfg'].abs().max()), 1e-3
        elif name == 'bn_nbt':
            err, bound = float(got != ref), 0.0
        elif name in ('s_out', 'f_out'):
            err, bound = float((got != ref).any()), 0.0            # the final states, bit for bit
        else:
            if name.startswith('dpre'):
                keep = ~info[int(name[4:])]['unreadable']
                got, ref = got * keep, ref * keep
            err, bound = fr.rel_err(got, ref), BOUND
        log(f'head_stage[{tag}].{stage}.{name}', err, bound)
        print(f'{tag} {stage:10s} {name:12s} {err:.3e} (bound {bound:g})')
        n += 1
        if not err <= bound:
            bad.append((stage, name, err))
    assert not bad, bad
    return n


def _forward_checks(tag, c, b, info):
    n = _check_pairs(tag, fr.head_fwd_stages(c), c, b, info)
    # per block xn mu rs q kv at o + the new state; yfg h1; bnm bni fus + 3 BatchNorm buffers; gw; 3 outputs
    assert n == 4 * 8 + 2 + 6 + 1 + 3, n


def _backward_checks(tag, c, b, info):
    n = _check_pairs(tag, fr.head_bwd_stages(c), c, b, info)
    assert n == 2 + 1 + 1 + 3 + 4 * 4 + 2 + 30, n
    dead = torch.ones(3, 3, dtype=torch.bool)
    dead[1, 1] = False
    assert float(b['g.wfg'][:, :, dead].abs().max()) == 0.0          # the fusion conv's 8 dead taps
    assert float(b['g.wfg'][:, :, 1, 1].abs().max()) > 0


@pytest.mark.parametrize('mx', [False, True])
@pytest.mark.parametrize('N', NS)
def test_head_forward_stages(N, mx):
    c, b, info = _run(N, mx)
    _forward_checks(f'N{N},{c.rounding}', c, b, info)


@pytest.mark.parametrize('mx', [False, True])
@pytest.mark.parametrize('N', NS)
def test_head_backward_stages(N, mx):
    """(a): dpre, dh1, dW2 and (through the stored dh1) dg1w are checked with the masks recovered
    from the forward (sites 0-3) and from dh1 (site 4, which the forward's gw check then shares)."""
    c, b, info = _run(N, mx)
    _backward_checks(f'N{N},{c.rounding}', c, b, info)


@pytest.mark.parametrize('mx', [False, True])
@pytest.mark.parametrize('N', NS)
def test_head_masks(N, mx):
    c, b, info = _run(N, mx)
    assert info[4]['ok'], 'a live gate unit whose dh1 / (dz2 W2) is neither 0 nor 1 / (1 - p)'
    for i in range(4):
        share = float(info[i]['small'].double().mean())
        log(f'head_mask[N{N},{c.rounding}].unreadable{i}', share, 0.01)
        assert share <= 0.01, (i, share)
    live, unread = info[4]['live'], info[4]['unreadable']
    log(f'head_mask[N{N},{c.rounding}].unreadable4', int(unread.sum()) / max(int(live.sum()), 1), 0.01)
    assert int(unread.sum()) <= 0.01 * int(live.sum())
    # (b) kept fraction within 5 binomial standard deviations of 1 - p
    for i in range(5):
        sel = info[i]['kept'] if i < 4 else info[4]['kept'][live]
        n = sel.numel()
        frac, sd = float(sel.double().mean()), (P_DROP * (1 - P_DROP) / n) ** 0.5
        log(f'head_mask[N{N},{c.rounding}].kept{i}', abs(frac - (1 - P_DROP)) / sd, 5.0)
        assert abs(frac - (1 - P_DROP)) <= 5 * sd, (i, frac, n)
    # (c) the five sites' masks are pairwise different
    for i in range(5):
        for j in range(i + 1, 5):
            a, d = info[i]['kept'], info[j]['kept']
            if j == 4:
                a, d = a[:, :64][live], d[live]
            assert not torch.equal(a, d), (i, j)
    # (d) frames n and n + 16 draw different masks: the index is built from the GLOBAL frame
    for i in range(4):
        k = info[i]['kept']
        for n in range(N - 16):
            assert not torch.equal(k[n], k[n + 16]), (i, n)
    # the gate site shows its mask on ReLU-live units only (a few dozen per frame pair, too few to
    # tell two frames apart one pair at a time): over all pairs, independent masks agree on
    # p^2 + (1 - p)^2 = 82 % of the units live in both frames, one shared mask on all of them
    if N > 16:
        both = live[:N - 16] & live[16:]
        agree = (info[4]['kept'][:N - 16] == info[4]['kept'][16:])[both].double()
        q = P_DROP ** 2 + (1 - P_DROP) ** 2
        assert float(agree.mean()) <= q + 5 * (q * (1 - q) / agree.numel()) ** 0.5, float(agree.mean())


@pytest.mark.parametrize('mx', [False, True])
def test_head_masks_change_with_the_step_counter(mx):
    """(e) after ewvit._lib.rng_advance every site draws another mask."""
    _, _, i0 = _run(37, mx, step=0)
    _, _, i1 = _run(37, mx, step=1)
    for i in range(4):
        assert not torch.equal(i0[i]['kept'], i1[i]['kept']), i
    both = i0[4]['live'] & i1[4]['live']
    assert not torch.equal(i0[4]['kept'][both], i1[4]['kept'][both])


@pytest.mark.parametrize('training,p', [(False, P_DROP), (True, 0.0)])
def test_head_eval_and_p0_all_kept(training, p):
    """(f) eval mode (the modules' p left at 0.1) and p = 0: every mask all-kept, nothing scaled —
    the stage checks hold with masks of exactly 1."""
    c, b, info = _run(37, False, training=training, p=p)
    for i in range(5):
        assert bool(info[i]['kept'].all()), i
        assert torch.equal(c.masks[i], torch.ones_like(c.masks[i])), i
    assert info[4]['ok']
    tag = f'N37,bf16,{"train" if training else "eval"},p{p}'
    _forward_checks(tag, c, b, info)
    _backward_checks(tag, c, b, info)
    if not training:
        assert b['bn_nbt'] == c.nbt and torch.equal(b['bn_rm'], c.rm) and torch.equal(b['bn_rv'], c.rv)


def _oracle_run(c, b, masks, N):
    """The float64 oracle modules with the kernel run's parameters and BatchNorm buffers and
    `masks` in place of their Dropouts: outputs, input and parameter gradients."""
    from test_fused_ref_cpu import OracleHead
    head = OracleHead().train()
    with torch.no_grad():
        for name, t in zip(fr.HEAD_PARAM_NAMES, head.params()):
            t.copy_(c.P[name])
        bn = head.fusion_gate[1]
        bn.running_mean.copy_(c.rm)
        bn.running_var.copy_(c.rv)
    head.set_masks(masks)
    s = b['st0'].clone().requires_grad_(True)
    f = b['st1'].clone().requires_grad_(True)
    out = head(s, f)
    (out['fused'] * b['g_fused'] + out['space'] * b['g_s'] + out['freq'] * b['g_f']).sum().backward()
    res = {'fused': out['fused'].detach(), 's_out': out['space'].detach(), 'f_out': out['freq'].detach(),
           'ds0': s.grad, 'df0': f.grad}
    for name, t in zip(fr.HEAD_PARAM_NAMES, head.params()):
        res['g.' + name] = t.grad
    return res


def _anchor_violations(tag, b, ref, do_log):
    bad = []
    for k in ('fused', 's_out', 'f_out'):
        err, c_ = fr.rel_err(b[k], ref[k]), cos(b[k], ref[k])
        if do_log:
            log(f'head_anchor[{tag}].{k}.err_of_scale', err, 2e-2)
            log(f'head_anchor[{tag}].{k}.cos', c_, 0.999)
        if not (err <= 2e-2 and c_ >= 0.999):
            bad.append((k, err, c_))
    for k in ['ds0', 'df0'] + ['g.' + n for n in fr.HEAD_PARAM_NAMES if n != 'bfg']:
        c_ = cos(b[k], ref[k])
        if do_log:
            log(f'head_anchor[{tag}].{k}.cos', c_, 0.99)
        if not c_ >= 0.99:
            bad.append((k, c_))
    return bad


@pytest.mark.parametrize('N', [64, 37])
def test_head_end_to_end_vs_oracle_with_recovered_masks(N):
    """bf16 form against the float64 oracle carrying the recovered masks: outputs 2e-2 of scale
    and cosine >= 0.999, input and parameter gradients cosine >= 0.99 (the project's oracle
    bounds; fusion_gate.0.bias is rounding noise on both sides and is left to the stage test).
    Negative control on the reference side only: with another step's masks the same comparison
    violates the bounds, so the anchor sees the mask."""
    c, b, _ = _run(N, False, step=0)
    bad = _anchor_violations(f'N{N}', b, _oracle_run(c, b, c.masks, N), True)
    assert not bad, bad
    c1, _, _ = _run(N, False, step=1)
    assert _anchor_violations(f'N{N}', b, _oracle_run(c, b, c1.masks, N), False)

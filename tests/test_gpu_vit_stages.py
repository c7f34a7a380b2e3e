"""The fused ViT encoder layer (csrc/vit.hip) checked stage by stage against float64, bf16 and
MXFP8 forms, to_out dropout 0.15 and 0.0, 64 / 37 / 1 frames (R = 2 x frames rows; 37 straddles
the kernels' 64-row halves).

ewvit_vit_layer_fwd / ewvit_vit_layer_bwd leave their intermediates in the `saved` and `scratch`
blobs.  Each stage is recomputed in float64 (tests/fused_ref.py, proven against the oracle on the
CPU in tests/test_fused_ref_cpu.py) from the kernel's own stored inputs to that stage, with the
operand rounding the kernel applies there.  Bounds: fp32 buffers max |err| <= 1e-4 of the
buffer's max |ref| (the project's bound for an fp32-accumulated product against a float64
emulation of the same rounded operands); buffers stored as bf16 |err| <= 2^-8 |ref| + 1e-4 of
scale against the UNROUNDED float64 value (one round-to-nearest of a value itself within the fp32
bound), logged as max (|err| - 2^-8 |ref|) / scale against 1e-4.  Everything measured goes to
EWVIT_PARITY_LOG.

Where the kernels round (read off csrc/vit.hip), and what follows for the checks:
* bf16 form: the GEMM operands LN1 / o / LN2 / g_o are formed in the A fragments from fp32 and
  also stored (transposed) as bf16 by a second evaluation of the same expression: the stored
  copy is taken as the operand (the nearest clean boundary);
* MXFP8 form: those four operands are quantized from the fp32 values, which are not stored.  They
  are recomputed in float64 from the stage's stored inputs; an element within 2^-18 (relative) of
  an e4m3 rounding boundary (or within the fp32 evaluation error of the operand's expression,
  where that is wider: small results of cancelling terms) could round either way.  Leaving out every row with such an
  element would drop ~4.5 % of the rows (K = 512; see test_fused_ref_cpu.py), above the 2 % cap, so
  each doubtful element is settled against the kernel's stored row instead (of its two roundings,
  the one that reproduces the row: fused_ref.resolve_rows); only rows that cannot be settled (a
  block maximum at the scale boundary, more than 4 doubtful elements) are left out, and those are
  asserted <= 2 % of the stage's rows;
* dh = g W2 and d(attention out) = g_o Wo are rounded to bf16 ("like the module path's") without
  being stored: g1 and dqkv are not clean boundaries (two roundings, the first of a value that is
  itself only within the fp32 bound of its reference, so which way it goes cannot be told).  They
  are checked from g / g_o with the first rounding's reach added to the bound: a perturbation of
  2^-8 |v| + 1e-4 of scale of dh / dO carried through GELU' / through the attention backward to
  first order in absolute values (fused_ref.bf16_mid_pert, attn_2x2_bwd_abs);
* the Linear1 bias partials db1p sum the unrounded fp32 g1, which is stored only as bf16: they
  are held to the stored g1 with the rigorous bound sum_r 2^-8 |g1| (one rounding per term)
  + 1e-4 of scale, and G.b1 to db1p[0] + db1p[1] at 1e-4;
* transposed copies (hT, g1T, dqkvT) must equal the row-major buffer bit for bit, and every
  transposed operand and LayerNorm row partial must be exactly zero past row R.

The to_out mask is recovered from x1 against x0 (kept iff x1 != x0), never generated; the few
elements equal in both whose pre-dropout value is below 1e-4 of scale cannot be read there (at
most 1 % asserted) and are read from the backward instead (g_o is exactly 0 iff dropped).  With it
injected, x1 (forward), goT / dbo / dqkv (backward) and dWo (weight gradient) are shown to use
one mask.
"""
import copy
import functools

import pytest
import torch

import fused_ref as fr
from test_gpu_modules import log

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F64 = torch.float64
BOUND = 1e-4
BF16_STORED = {'ln1', 'qkv', 'o', 'ln2', 'aux', 'h', 'g1', 'go', 'dqkv', 'gT'}
BS = [64, 37, 1]


@functools.lru_cache(maxsize=None)
def _base(drop):
    from test_gpu_vit import _vit
    return _vit(drop).train()


@functools.lru_cache(maxsize=None)
def _run(B, mx, drop):
    """One forward + backward of ViTLayerFn on layer 0; everything it wrote, on the CPU."""
    import ewvit
    from ewvit import vit as ev
    L = ewvit._lib
    m = copy.deepcopy(_base(drop))
    attn, ff = m.layers[0]
    ts = ev.params_of(attn, ff)
    R = 2 * B
    xc, gc = fr.vit_inputs(B)
    x0 = xc.to(DEV).requires_grad_(True)
    L.rng_offset(x0.device).zero_()      # a fixed step counter: the mask does not depend on what ran before
    L.rng_advance(x0.device)
    buf = ev.pack([(attn, ff)], mx=mx)
    x2 = ev.ViTLayerFn.apply((attn.norm.eps, float(drop), 4242 if drop > 0 else 0, buf, 0, mx), x0, *ts)
    saved = x2.grad_fn.saved_tensors[1]
    scratch = torch.zeros(int(L.load().ewvit_vit_layer_workspace(1)), dtype=torch.uint8, device=DEV)
    real = L.call

    def call(name, *args, **kw):         # the backward allocates its scratch itself: hand it ours
        if name == 'ewvit_vit_layer_bwd':
            args = args[:5] + (L.ptr(scratch),) + args[6:]
        return real(name, *args, **kw)
    L.call = call
    try:
        x2.backward(gc.to(DEV))
    finally:
        L.call = real
    torch.cuda.synchronize()
    S = fr.vit_saved_views(saved.cpu().clone(), int(L.load().ewvit_vit_layer_workspace(0)))
    Z = fr.vit_scratch_views(scratch.cpu().clone(), int(L.load().ewvit_vit_layer_workspace(1)))
    d = lambda t: t.to(F64)
    b = {'x0': d(xc.reshape(R, 512)), 'g': d(gc.reshape(R, 512)), 'x2': d(x2.detach().cpu().reshape(R, 512)),
         'dx0': d(x0.grad.cpu().reshape(R, 512)),
         'ln1': d(S['ln1T'].t()[:R]), 'o': d(S['oT'].t()[:R]), 'ln2': d(S['ln2T'].t()[:R]),
         'go': d(Z['goT'].t()[:R]), 'gT': d(Z['gT'].t()[:R])}
    for k in ('mu1', 'rs1', 'mu2', 'rs2', 'p', 'x1', 'qkv', 'aux', 'h'):
        b[k] = d(S[k][:R])
    for k in ('g1', 'dqkv', 'dln2', 'dx1', 'dln1'):
        b[k] = d(Z[k][:R])
    for name, t in zip(fr.VIT_PARAM_NAMES, ts):
        b['g.' + name] = d(t.grad.detach().cpu())
    c = fr.VitCfg(fr.vit_params(ts), None, 'mx' if mx else 'bf16', attn.norm.eps)
    # the to_out mask from the forward: kept iff x1 != x0 (fp32, as stored)
    c.mask = torch.ones(R, 512, dtype=F64)
    pre = dict(fr.vit_fwd_stages(c))['out'](b)['pre1']
    c.mask, kept, unreadable, small = fr.recover_ca_mask(xc.reshape(R, 512), S['x1'][:R], pre, drop)
    # an element equal in x1 and x0 whose pre-dropout value is too small to tell (a handful): read
    # from the backward instead, where a dropped element's g_o is exactly 0
    kept = torch.where(unreadable, Z['goT'].t()[:R].float() != 0, kept)
    c.mask = kept.to(F64) / (1.0 - drop)
    return c, b, S, Z, {'kept': kept, 'unreadable': unreadable, 'small': small}


def _judge(tag, stage, name, got, ref, keep, bad, extra=None):
    """One buffer against its float64 stage value; keep: rows that take part; extra: what an
    unstored bf16 rounding inside the stage may add (fused_ref 'pert.<name>')."""
    if keep is not None:
        got, ref = got * keep, ref * keep
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    if extra is not None:
        err = (err - extra).clamp_min(0)
    if name in BF16_STORED:
        err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0)
    v = float(err.max()) / scale if scale > 0 else float(err.max())
    log(f'vit_stage[{tag}].{stage}.{name}', v, BOUND)
    print(f'{tag} {stage:9s} {name:9s} {v:.3e} (bound {BOUND:g}{", bf16-stored" if name in BF16_STORED else ""})')
    if not v <= BOUND:
        bad.append((stage, name, v))


def _settle(c, b, key, fn, Wk, post, got, R, tag):
    """MX form: the operand of stage output `key` with its doubtful roundings settled against the
    kernel's stored rows; returns the rows left out."""
    res = fn(b)
    q, alts, left = fr.mx_alternatives(res['opnd.' + key], abs_tol=res['tol.' + key])
    c.override[key] = fr.resolve_rows(q, alts, left, fr.mxq(Wk), post, got)
    log(f'vit_stage[{tag}].left_out_rows.{key}', int(left.sum()) / R, 0.02)
    log(f'vit_stage[{tag}].settled_rows.{key}', len(alts) / R, 1.0)
    assert int(left.sum()) <= 0.02 * R, (key, int(left.sum()))
    return (~left).to(F64)[:, None]


def _stage_checks(B, mx, drop):
    c, b, S, Z, info = _run(B, mx, drop)
    c.override = {}
    R, P = 2 * B, c.P
    tag = f'B{B},{c.rounding},p{drop}'
    bad, keep = [], {}
    fwd, bwd = dict(fr.vit_fwd_stages(c)), dict(fr.vit_bwd_stages(c))
    if mx:
        keep['qkv'] = _settle(c, b, 'qkv', fwd['qkv'], P['wqkv'], lambda r, o: o, lambda r: b['qkv'][r], R, tag)
        keep['x1'] = _settle(c, b, 'x1', fwd['out'], P['wo'], lambda r, o: b['x0'][r] + (o + P['bo']) * c.mask[r],
                             lambda r: b['x1'][r], R, tag)
        keep['aux'] = keep['h'] = _settle(c, b, 'aux', fwd['mlp1'], P['w1'], lambda r, o: o + P['b1'],
                                          lambda r: b['aux'][r], R, tag)

        def post_dqkv(r, o):              # the frame's attention backward with this row's d(attention out)
            f = r // 2
            do = q0[2 * f:2 * f + 2] @ wq.t()
            do[r & 1] = o
            return fr.attn_2x2_bwd(do, b['qkv'][2 * f:2 * f + 2], b['p'][2 * f:2 * f + 2])
        q0, wq = fr.mxq(b['dx1'] * c.mask), fr.mxq(P['wo'].t())
        keep['dqkv'] = _settle(c, b, 'dqkv', bwd['attn_bwd'], P['wo'].t(), post_dqkv,
                               lambda r: b['dqkv'][2 * (r // 2):2 * (r // 2) + 2], R, tag)
        keep['dqkv'] = keep['dqkv'].view(B, 2, 1).amin(1, keepdim=True).expand(B, 2, 1).reshape(R, 1)
    n = 0
    for stage, fn in fr.vit_fwd_stages(c) + fr.vit_bwd_stages(c):
        res = fn(b)
        for name, ref in res.items():
            if name not in b or name == 'g.b1' or name.startswith(fr.AUX_NAMES):
                continue
            _judge(tag, stage, name, b[name], ref, keep.get(name), bad, res.get('pert.' + name))
            n += 1
    assert n == 13 + 7 + 10, n
    # ---- what the kernels keep besides: transposed copies, partial sums, zero padding
    z = lambda t: float(t.float().abs().max()) if t.numel() else 0.0
    for name, T, rows in (('hT', S['hT'], S['h']), ('g1T', Z['g1T'], Z['g1']), ('dqkvT', Z['dqkvT'], Z['dqkv'])):
        assert torch.equal(T[:, :R], rows[:R].t()), name
    for name, T in (('ln1T', S['ln1T']), ('oT', S['oT']), ('ln2T', S['ln2T']), ('hT', S['hT']), ('gT', Z['gT']),
                    ('g1T', Z['g1T']), ('goT', Z['goT']), ('dqkvT', Z['dqkvT'])):
        assert z(T[:, R:]) == 0.0, (name, 'rows past R')
    for name in ('rp2', 'rp1'):
        assert z(Z[name][:, R:]) == 0.0, (name, 'rows past R')
    for name in ('mu1', 'rs1', 'mu2', 'rs2'):
        assert z(S[name][R:]) == 0.0, name
    _judge(tag, 'B2', 'rp2', Z['rp2'][:, :R].to(F64),
           fr.ln_row_partials(b['dln2'], b['x1'], b['mu2'], b['rs2'], P['ln2_w']), None, bad)
    _judge(tag, 'B4', 'rp1', Z['rp1'][:, :R].to(F64),
           fr.ln_row_partials(b['dln1'], b['x0'], b['mu1'], b['rs1'], P['ln1_w']), None, bad)
    _judge(tag, 'B1', 'gT', b['gT'], b['g'], None, bad)
    db1p = Z['db1p'].to(F64)
    _judge(tag, 'B2', 'g.b1', b['g.b1'], db1p[0] + db1p[1], None, bad)
    halves = torch.stack([b['g1'][:64].sum(0), b['g1'][64:].sum(0)])
    slack = 2.0 ** -8 * 1.01 * torch.stack([b['g1'][:64].abs().sum(0), b['g1'][64:].abs().sum(0)])
    v = float(((db1p - halves).abs() - slack).clamp_min(0).max()) / float(halves.abs().max())
    log(f'vit_stage[{tag}].B1.db1p', v, BOUND)
    print(f'{tag} B1        db1p      {v:.3e} (bound {BOUND:g} beyond the stored g1\'s roundings)')
    if not v <= BOUND:
        bad.append(('B1', 'db1p', v))
    assert not bad, bad
    return c, info


@pytest.mark.parametrize('drop', [0.15, 0.0])
@pytest.mark.parametrize('mx', [False, True])
@pytest.mark.parametrize('B', BS)
def test_vit_stages(B, mx, drop):
    c, info = _stage_checks(B, mx, drop)
    R = 2 * B
    share = float(info['small'].double().mean())
    log(f'vit_mask[B{B},{c.rounding},p{drop}].unreadable', share, 0.01)
    assert share <= 0.01, share
    kept = info['kept']
    if drop == 0:
        assert bool(kept.all()) and torch.equal(c.mask, torch.ones_like(c.mask))
    else:
        frac, sd = float(kept.double().mean()), (drop * (1 - drop) / kept.numel()) ** 0.5
        log(f'vit_mask[B{B},{c.rounding},p{drop}].kept', abs(frac - (1 - drop)) / sd, 5.0)
        assert abs(frac - (1 - drop)) <= 5 * sd, (frac, kept.numel())
        for r in range(R - 32):          # rows a workgroup-local index would give one mask
            assert not torch.equal(kept[r], kept[r + 32]) and (r + 64 >= R or not torch.equal(kept[r], kept[r + 64])), r

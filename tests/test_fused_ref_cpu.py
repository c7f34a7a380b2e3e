"""The float64 stage references of tests/fused_ref.py checked against the oracle on the CPU,
independently of the kernels they are the yardstick for.

* The head stages chained (no rounding) reproduce oracle.model's BidirectionalCrossTransformer +
  fusion_gate + gate_net + weighted sum (DAMA.fuse) in .double(), on recipe weights: outputs
  and BatchNorm buffers to 1e-10 of scale, the hand-written backward against torch autograd to
  1e-9 of scale for both inputs and all 32 parameters — with all-ones masks, and with a fixed
  non-trivial mask against the oracle with its Dropout modules replaced by that mask.
* The same for the ViT layer stages against oracle.model.Transformer(512, 1, 8, 64, 2048, 0.0).
* The caps the GPU stage tests assert (unreadable mask elements, rows left out next to an MXFP8
  rounding boundary) hold for the reference alone at the tests' input seeds.
* Each stage check bites: a corrupted copy of a stage's stored output (a frame's mask shifted by
  16 rows, one K block's scale doubled, the last ragged frame dropped from a weight-gradient
  sum) fails the 1e-4 bound the GPU tests hold the kernels to.
"""
import pytest
import torch
from torch import nn

import fused_ref as fr

F64 = torch.float64
STAGE_BOUND = 1e-4


# ---------------------------------------------------------------- the oracle head
class _Mask(nn.Module):
    """Stands in for a Dropout: multiplies by a fixed mask (already scaled by 1 / (1 - p))."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.view(x.shape)


class OracleHead(nn.Module):
    """The head's modules as oracle.model.DAMA builds them (dama.py:105-128), without the two
    branches; `fuse` is the oracle's own."""

    def __init__(self, seed=3, dim=128, heads=4):
        super().__init__()
        from oracle import model as om
        from oracle.weights import apply_recipe
        self.gate_net = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(2 * dim, dim // 2),
                                      nn.ReLU(), nn.Dropout(0.1), nn.Linear(dim // 2, 3), nn.Softmax(dim=1))
        self.cross_att = om.BidirectionalCrossTransformer(dim, depth=2, heads=heads, dim_head=dim // heads, dropout=0.1)
        self.fusion_gate = nn.Sequential(nn.Conv2d(dim * 2, dim, 3, padding=1), nn.BatchNorm2d(dim),
                                         nn.ReLU(inplace=True))
        apply_recipe(self, seed)
        self.double()

    def set_masks(self, masks):
        """masks {0..3: [N, 128], 4: [N, 64]} in place of the five Dropouts (kernel site order)."""
        for i in range(4):
            self.cross_att.layers[i >> 1][1 + 2 * (i & 1)].to_out[1] = _Mask(masks[i])
        self.gate_net[4] = _Mask(masks[4])

    def forward(self, s, f):
        from oracle import model as om
        N = s.shape[0]
        return om.DAMA.fuse(self, s.view(N, -1, 1, 1), f.view(N, -1, 1, 1))

    def params(self):
        return fr.head_param_list(self.cross_att, self.fusion_gate, self.gate_net)


def _masks(N, p, seed):
    if p == 0:
        return {i: torch.ones(N, 64 if i == 4 else 128, dtype=F64) for i in range(5)}
    g = torch.Generator().manual_seed(seed)
    return {i: (torch.rand(N, 64 if i == 4 else 128, generator=g) >= p).to(F64) / (1 - p) for i in range(5)}


def _head_cfg(head, masks, rounding, training):
    bn = head.fusion_gate[1]
    return fr.HeadCfg(fr.head_params(head.params()), masks, rounding, training,
                      (bn.running_mean.clone().to(F64), bn.running_var.clone().to(F64), int(bn.num_batches_tracked),
                       bn.momentum, bn.eps), head.cross_att.layers[0][0].eps)


def _head_ref(head, N, masks, rounding, training=True):
    """The reference chain, forward and backward, on the head tests' inputs."""
    s0, f0, gs = fr.head_inputs(N)
    c = _head_cfg(head, masks, rounding, training)
    b = {'st0': s0.to(F64), 'st1': f0.to(F64), 'g_fused': gs[0].to(F64), 'g_s': gs[1].to(F64), 'g_f': gs[2].to(F64)}
    fr.run_chain(fr.head_fwd_stages(c), b)
    if training:
        fr.run_chain(fr.head_bwd_stages(c), b)
    return c, b


@pytest.mark.parametrize('N,p', [(37, 0.0), (37, 0.1), (5, 0.1), (64, 0.3)])
def test_head_stages_chain_to_the_oracle(N, p):
    head = OracleHead().train()
    masks = _masks(N, p, 11 + N)
    _, b = _head_ref(head, N, masks, None)            # (reads the BatchNorm buffers before the oracle runs)
    head.set_masks(masks)
    s0, f0, gs = fr.head_inputs(N)
    s = s0.to(F64).requires_grad_(True)
    f = f0.to(F64).requires_grad_(True)
    out = head(s, f)
    for k, name in (('fused', 'fused'), ('space', 's_out'), ('freq', 'f_out')):
        assert fr.rel_err(b[name], out[k].detach()) <= 1e-10, k
    bn = head.fusion_gate[1]
    assert fr.rel_err(b['bn_rm'], bn.running_mean) <= 1e-10 and fr.rel_err(b['bn_rv'], bn.running_var) <= 1e-10
    assert b['bn_nbt'] == int(bn.num_batches_tracked) == 1
    (out['fused'] * gs[0].to(F64) + out['space'] * gs[1].to(F64) + out['freq'] * gs[2].to(F64)).sum().backward()
    assert fr.rel_err(b['ds0'], s.grad) <= 1e-9 and fr.rel_err(b['df0'], f.grad) <= 1e-9
    scale_fg = float(head.fusion_gate[0].weight.grad.abs().max())
    for name, t in zip(fr.HEAD_PARAM_NAMES, head.params()):
        if name == 'bfg':      # feeds a train-mode BatchNorm: an exact zero, rounding noise on both sides
            assert float(b['g.bfg'].abs().max()) <= 1e-9 * scale_fg and float(t.grad.abs().max()) <= 1e-9 * scale_fg
            continue
        assert fr.rel_err(b['g.' + name], t.grad) <= 1e-9, name
    dead = torch.ones(3, 3, dtype=torch.bool)
    dead[1, 1] = False
    assert float(b['g.wfg'][:, :, dead].abs().max()) == 0.0
    assert float(head.fusion_gate[0].weight.grad[:, :, dead].abs().max()) == 0.0


def test_head_stages_chain_to_the_oracle_eval():
    N = 17
    head = OracleHead().eval()
    _, b = _head_ref(head, N, _masks(N, 0.0, 0), None, training=False)
    s0, f0, _ = fr.head_inputs(N)
    with torch.no_grad():
        out = head(s0.to(F64), f0.to(F64))
    for k, name in (('fused', 'fused'), ('space', 's_out'), ('freq', 'f_out')):
        assert fr.rel_err(b[name], out[k]) <= 1e-10, k
    assert b['bn_nbt'] == 0 and torch.equal(b['bn_rm'], head.fusion_gate[1].running_mean)


def test_head_layout_is_the_kernels():
    """W_TOTAL of csrc/head.hip as its constants state it (the GPU tests compare the same number
    with ewvit_head_workspace())."""
    HN, HD = 64, 128
    blk = HN * HD + 2 * HN + HN * HD + HN * 512 + HN * 8 + HN * HD
    fus0 = 6 * HN * HD + 4 * blk
    bblk0 = fus0 + HN * HD + 2 * HD + HN * HD + HN * 64 + HN * 4
    tail0 = bblk0 + 4 * (HN * HD + HN * HD + HN * 512 + HN * HD)
    total = tail0 + HN * HD + HN * 64 + HN * 4 + 2 * HN * HD + HD * 256 + 256
    lay, n = fr.head_layout()
    assert n == total
    off = {name: o for name, o, _ in lay}
    assert off['yfg'] == fus0 and off['dxn0'] == bblk0 and off['dy'] == tail0 and off['xn0'] == 6 * HN * HD
    ws = torch.arange(total, dtype=torch.float32)
    v = fr.head_ws_views(ws, total * 4, N=5)
    assert v['kv1'].shape == (5, 2, 256) and float(v['q1'][0, 0]) == off['q1']
    with pytest.raises(AssertionError):
        fr.head_ws_views(ws, total * 4 + 4)


# ---------------------------------------------------------------- caps, on the tests' seeds
@pytest.mark.parametrize('N', [64, 37, 17, 5])
@pytest.mark.parametrize('rounding', ['bf16', 'mx'])
def test_head_mask_recovery_caps_hold_for_the_reference(N, rounding):
    """The reference alone, with a known mask, at the GPU test's inputs: both recoveries return
    the mask that was applied wherever they can read it, and the unreadable share of every site is
    under the 1 % the GPU test asserts.  (Rounded operands: the reference's buffers then behave
    as the kernel's do; the comparison st_out != st_in is made in fp32 as the kernel stores it.)"""
    p = 0.1
    head = OracleHead().train()
    masks = _masks(N, p, 5 + N)
    c, b = _head_ref(head, N, masks, rounding)
    for i in range(4):
        st_in, st_out = b[f'st{fr.h_xin(i)}'].float(), b[f'st{fr.h_xout(i)}'].float()
        m, kept, unreadable, small = fr.recover_ca_mask(st_in, st_out, b[f'pre{i}'], p)
        assert float(small.double().mean()) <= 0.01, (i, float(small.double().mean()))
        assert torch.equal(kept[~unreadable], masks[i][~unreadable] > 0), i
    m, kept, live, unreadable, ok = fr.recover_gate_mask(b['dh1'], b['dz2'], b['h1'], c.P['g1b'], c.P['g2w'], p)
    assert ok
    assert int(unreadable.sum()) <= 0.01 * int(live.sum())
    readable = live & ~unreadable
    assert torch.equal(kept[readable], masks[4][readable] > 0)


# ---------------------------------------------------------------- the stage checks bite
def _worst(stages, b, only=None):
    return {name: fr.rel_err(got, ref) for _, name, got, ref in fr.stage_pairs(stages, b)
            if only is None or name in only}


def test_head_stage_check_is_clean_on_the_reference_and_bites():
    """On the reference's own buffers (bf16 operands, N = 37) every stage check is at float64
    noise.  Then three corruptions of a copy of a stored output, each far over the 1e-4 bound:
    one frame's to_out mask taken from 16 frames on (the workgroup-local row), the last ragged
    frame left out of a weight-gradient sum, one 32-wide K block of an MX operand scaled 2x."""
    N, p = 37, 0.1
    head = OracleHead().train()
    masks = _masks(N, p, 42)
    c, b = _head_ref(head, N, masks, 'bf16')
    fwd, bwd = fr.head_fwd_stages(c), fr.head_bwd_stages(c)
    clean = {**_worst(fwd, b), **_worst(bwd, b)}
    assert len(clean) == 44 + 55, len(clean)
    assert max(clean.values()) <= 1e-12, max(clean.items(), key=lambda kv: kv[1])

    # (1) frame 20 of block 2 written with frame 36's mask (20 + 16): forward and backward
    bad = dict(b)
    m = masks[2].clone()
    m[20] = masks[2][36]
    assert not torch.equal(m[20], masks[2][20])
    bad['st4'] = b['st2'] + b['pre2'] * m
    assert _worst(fwd, bad, {'st4'})['st4'] > STAGE_BOUND
    bad = dict(b)
    bad['dpre2'] = fr._head_streams(c, b, 2)[0] * m
    assert _worst(bwd, bad, {'dpre2'})['dpre2'] > STAGE_BOUND

    # (2) the ragged last frame (36) dropped from to_q's weight gradient of block 1
    bad = dict(b)
    bad['g.ca1.wq'] = fr.wgrad(b['dq1'][:N - 1], b['xn1'][:N - 1], 'bf16')
    assert _worst(bwd, bad, {'g.ca1.wq'})['g.ca1.wq'] > STAGE_BOUND

    # (3) MXFP8: K block 1 (columns 32..63) of one frame's LayerNorm row scaled 2x in to_q
    c8, b8 = _head_ref(head, N, masks, 'mx')
    fwd8 = fr.head_fwd_stages(c8)
    assert max(_worst(fwd8, b8).values()) <= 1e-12
    xq = fr._opnd(b8['xn0'], 'mx', True).clone()
    xq[7, 32:64] *= 2
    bad = dict(b8)
    bad['q0'] = xq @ fr._opnd(c8.P['ca0.wq'], 'mx', False).t()
    assert _worst(fwd8, bad, {'q0'})['q0'] > STAGE_BOUND


# ================================================================ the ViT layer
def _oracle_vit(seed=3):
    from oracle import model as om
    from oracle.weights import apply_recipe
    return apply_recipe(om.Transformer(512, 1, 8, 64, 2048, 0.0), seed).double().train()


def _vit_ref(tr, B, mask, rounding):
    x, g = fr.vit_inputs(B)
    attn, ff = tr.layers[0]
    c = fr.VitCfg(fr.vit_params(fr.vit_param_list(attn, ff)), mask, rounding, attn.norm.eps)
    b = {'x0': x.reshape(2 * B, 512).to(F64), 'g': g.reshape(2 * B, 512).to(F64)}
    fr.run_chain(fr.vit_fwd_stages(c), b)
    fr.run_chain(fr.vit_bwd_stages(c), b)
    return c, b


def _vit_mask(B, p, seed):
    if p == 0:
        return torch.ones(2 * B, 512, dtype=F64)
    return (torch.rand(2 * B, 512, generator=torch.Generator().manual_seed(seed)) >= p).to(F64) / (1 - p)


@pytest.mark.parametrize('B,p', [(37, 0.0), (37, 0.15), (1, 0.15)])
def test_vit_stages_chain_to_the_oracle(B, p):
    tr = _oracle_vit()
    mask = _vit_mask(B, p, 9 + B)
    _, b = _vit_ref(tr, B, mask, None)
    attn, ff = tr.layers[0]
    attn.fn.to_out[1] = _Mask(mask.view(B, 2, 512))
    x, g = fr.vit_inputs(B)
    xo = x.to(F64).requires_grad_(True)
    y = tr(xo)
    assert fr.rel_err(b['x2'], y.detach().reshape(2 * B, 512)) <= 1e-10
    (y * g.to(F64)).sum().backward()
    assert fr.rel_err(b['dx0'], xo.grad.reshape(2 * B, 512)) <= 1e-9
    for name, t in zip(fr.VIT_PARAM_NAMES, fr.vit_param_list(attn, ff)):
        assert fr.rel_err(b['g.' + name], t.grad) <= 1e-9, name


def test_vit_layout_is_the_kernels():
    """saved_layout / scratch_layout of csrc/vit.hip as its `put` calls state them."""
    def al(n):
        return (n + 255) // 256 * 256
    R, D, Q, F, H = 128, 512, 1536, 2048, 8
    saved = 4 * al(4 * R) + al(4 * R * H * 2) + al(4 * R * D) + al(2 * R * Q) + 2 * al(2 * R * F) + 3 * al(2 * D * R) + \
        al(2 * F * R) + al(4 * 16 * R * D)
    scratch = al(2 * D * R) + al(2 * R * F) + al(2 * F * R) + al(2 * D * R) + al(2 * R * Q) + al(2 * Q * R) + \
        3 * al(4 * R * D) + 2 * al(4 * 32 * R * 2) + al(4 * 2 * F)
    assert fr.vit_layout_bytes() == (saved, scratch)
    v = fr.vit_saved_views(torch.zeros(saved, dtype=torch.uint8), saved)
    assert v['qkv'].shape == (128, 1536) and v['qkv'].dtype == torch.bfloat16 and v['x1'].dtype == torch.float32
    with pytest.raises(AssertionError):
        fr.vit_scratch_views(torch.zeros(scratch, dtype=torch.uint8), scratch + 256)


@pytest.mark.parametrize('B', [64, 37, 1])
def test_vit_mx_left_out_rows_cap_holds_for_the_reference(B):
    """The operands the MXFP8 form quantizes from fp32 values it does not store (LN1, the
    attention output, LN2, to_out's output gradient), from the reference alone at the GPU test's
    inputs.  A row of K = 512 holds an element within 2^-18 (relative) of an e4m3 rounding
    boundary with probability ~4.5 % (measured here: 2.3-9.5 % of the rows), so leaving such rows
    out would exceed the 2 % cap the GPU test asserts: the GPU test instead settles each doubtful
    element against the kernel's stored row (fused_ref.mx_alternatives / resolve_rows) and leaves
    out only the rows that cannot be settled that way.  Those are at most 2 % of the rows; and
    resolving against the reference's own output picks the reference's own rounding back."""
    tr = _oracle_vit()
    c, b = _vit_ref(tr, B, _vit_mask(B, 0.15, 3), 'mx')
    res = {}
    for _, fn in fr.vit_fwd_stages(c) + fr.vit_bwd_stages(c):
        res.update(fn(b))
    for name in ('opnd.qkv', 'opnd.x1', 'opnd.aux', 'opnd.dqkv'):
        q, alts, left = fr.mx_alternatives(res[name])
        assert int(left.sum()) <= 0.02 * 2 * B, (name, int(left.sum()))
        assert len(alts) <= 0.12 * 2 * B + 1, (name, len(alts))
    q, alts, left = fr.mx_alternatives(res['opnd.qkv'])
    Wq = fr.mxq(c.P['wqkv'])
    q2 = fr.resolve_rows(q, alts, left, Wq, lambda r, o: o, lambda r: b['qkv'][r])
    assert torch.equal(q2, q)
    if alts:                      # the other rounding of one doubtful element: found again from the output
        r, (k, d) = next((r, cand[0]) for r, cand in alts.items())
        flipped = q.clone()
        flipped[r, k] += d
        got = flipped @ Wq.t()
        assert fr.rel_err(got, b['qkv']) > STAGE_BOUND          # ... and it matters at the stage bound
        assert torch.equal(fr.resolve_rows(q, alts, left, Wq, lambda r, o: o, lambda r: got[r]), flipped)


def test_vit_stage_check_is_clean_on_the_reference_and_bites():
    """bf16 and MX operands, B = 37: every stage check is at float64 noise on the reference's own
    buffers; one 32-wide K block of to_qkv's MX operand scaled 2x, or the last frame's two rows
    dropped from Linear2's weight gradient, fails the 1e-4 bound."""
    B = 37
    tr = _oracle_vit()
    for rounding in ('bf16', 'mx'):
        c, b = _vit_ref(tr, B, _vit_mask(B, 0.15, 3), rounding)
        stages = fr.vit_fwd_stages(c) + fr.vit_bwd_stages(c)
        clean = _worst(stages, b)
        assert len(clean) == 13 + 7 + 11, sorted(clean)
        assert max(clean.values()) <= 1e-12, max(clean.items(), key=lambda kv: kv[1])
    xq = fr.mxq(fr.layernorm(b['x0'], c.P['ln1_w'], c.P['ln1_b'], c.ln_eps)[0]).clone()
    xq[2 * B - 1, 64:96] *= 2
    bad = dict(b)
    bad['qkv'] = xq @ fr.mxq(c.P['wqkv']).t()
    assert _worst(stages, bad, {'qkv'})['qkv'] > STAGE_BOUND
    bad = dict(b)
    bad['g.w2'] = fr.wgrad(b['g'][:2 * B - 2], b['h'][:2 * B - 2], 'mx')
    assert _worst(stages, bad, {'g.w2'})['g.w2'] > STAGE_BOUND

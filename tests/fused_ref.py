"""Float64 stage references for the two fused token kernels (a helper module, not a test).

csrc/head.hip (the DAMA frame head) and csrc/vit.hip (one ViT encoder layer) leave every
intermediate in their workspaces.  This module gives

* views of those workspaces by name (`head_ws_views`, `vit_saved_views`, `vit_scratch_views`),
  each checked against the byte count the library reports, so a layout change in a kernel cannot
  silently shift a view;
* every stage of both kernels, forward and hand-derived backward, in float64 on plain tensors,
  written from the reference's semantics:
    network/dama.py:15-78    CrossAttention / BidirectionalCrossTransformer (the four blocks),
    network/dama.py:105-128  gate_net and fusion_gate,
    network/dama.py:143-169  the per-frame head (concat, fusion conv on the 1x1 map, gate, sum),
    network/sfe.py:20-85     PreNorm / FeedForward / Attention / Transformer (the ViT layer);
* the stages strung together as a list (`head_fwd_stages`, `head_bwd_stages`, ...).  A stage
  reads its inputs by name from a dict of buffers and returns its outputs by name, so the same
  definition serves as a chain (`run_chain`: each stage fed by the one before — the whole
  operation, compared with the oracle modules in tests/test_fused_ref_cpu.py) and as a stage
  check (`stage_pairs`: each stage fed by the KERNEL's stored inputs to that stage and compared
  with the kernel's stored output, so errors do not compound).

Operand rounding is an argument of every GEMM stage: None (exact), 'bf16' (both operands
rounded to bf16, as `A1[..] = f2bf(y0)` next to `ws.xn = y0` in head_fwd_rows_kernel) or 'mx'
(MXFP8 blocks of 32 along the GEMM's K, `_mx_q` of tests/test_gpu_fp8.py, which is pinned
bit-level against ewvit_gemm_mx8).  Dropout enters as explicit masks already scaled by
1 / (1 - p) (0 for a dropped element); nothing here generates random numbers, and the kernels'
counter-based generator is deliberately not restated: the GPU tests recover the masks from what
the kernels wrote (`recover_ca_mask`, `recover_gate_mask`).

Nothing in this module calls into ewvit.
"""
import torch

F64 = torch.float64


# ---------------------------------------------------------------- operand rounding
def bf16(x):
    return x.float().bfloat16().to(F64)


def mxq(x):
    """MXFP8 of x [R, K] along K in float64 (tests/test_gpu_fp8.py)."""
    from test_gpu_fp8 import _mx_q
    return _mx_q(x.float()).to(F64)


def _opnd(x, rounding, via_bf16):
    """A GEMM operand [rows, K] under `rounding`; via_bf16: an MX operand the kernel quantizes
    from a bf16 copy (the head's LDS rows) instead of from the fp32 value."""
    if rounding is None:
        return x.to(F64)
    if rounding == 'bf16':
        return bf16(x)
    assert rounding == 'mx', rounding
    return mxq(bf16(x) if via_bf16 else x)


def linear(x, W, rounding=None, act_via_bf16=True):
    """y = x W^T (nn.Linear without bias): x [R, K], W [O, K], K the reduction."""
    return _opnd(x, rounding, act_via_bf16) @ _opnd(W, rounding, False).t()


def dgrad(g, W, rounding=None, act_via_bf16=True):
    """dx = g W: g [R, O], W [O, K]; the reduction runs over O (the kernel reads W^T)."""
    return _opnd(g, rounding, act_via_bf16) @ _opnd(W.t(), rounding, False).t()


def wgrad(d, x, rounding=None, rows=None):
    """dW = d^T x over the rows (frames): d [R, O], x [R, K] -> [O, K].  MX blocks run along the
    rows, zero-padded to `rows` (the kernel's fixed frame count), quantized from the fp32 values."""
    if rounding == 'mx' and rows is not None and d.shape[0] < rows:
        pad = rows - d.shape[0]
        d = torch.cat([d, d.new_zeros(pad, d.shape[1])])
        x = torch.cat([x, x.new_zeros(pad, x.shape[1])])
    return _opnd(d.t(), rounding, False) @ _opnd(x.t(), rounding, False).t()


# ---------------------------------------------------------------- elementwise stages
def layernorm(x, w, b, eps):
    """torch.nn.LayerNorm over the last dim: biased variance, eps inside the root."""
    mu = x.mean(-1)
    rs = 1.0 / torch.sqrt(((x - mu[:, None]) ** 2).mean(-1) + eps)
    return (x - mu[:, None]) * rs[:, None] * w + b, mu, rs


def layernorm_bwd(dy, x, mu, rs, w):
    """-> dx, dw, db.  dx = rs (g - mean(g) - xhat mean(g xhat)), g = dy w."""
    xh = (x - mu[:, None]) * rs[:, None]
    g = dy * w
    dx = rs[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def attn_1x2(q, kv, heads=4):
    """One query against two keys per (frame, head) (dama.py:37-50 with kv_include_self on one
    token per stream): q [N, D], kv [N, 2, 2D] (token 0 = the normed self token, 1 = the context;
    k in [:D], v in [D:]) -> softmax weights [N, heads, 2], output [N, D]."""
    N, D = q.shape
    dh = D // heads
    qh = q.view(N, heads, dh)
    k = kv[:, :, :D].reshape(N, 2, heads, dh)
    v = kv[:, :, D:].reshape(N, 2, heads, dh)
    dots = torch.einsum('nhd,njhd->nhj', qh, k) * dh ** -0.5
    a = torch.softmax(dots, -1)
    return a, torch.einsum('nhj,njhd->nhd', a, v).reshape(N, D)


def attn_1x2_bwd(do, q, kv, a, heads=4):
    """-> dq [N, D], dkv [N, 2, 2D] from the stored q, kv and softmax weights a."""
    N, D = q.shape
    dh = D // heads
    qh, doh = q.view(N, heads, dh), do.view(N, heads, dh)
    k = kv[:, :, :D].reshape(N, 2, heads, dh)
    v = kv[:, :, D:].reshape(N, 2, heads, dh)
    da = torch.einsum('nhd,njhd->nhj', doh, v)
    dl = a * (da - (a * da).sum(-1, keepdim=True)) * dh ** -0.5
    dq = torch.einsum('nhj,njhd->nhd', dl, k).reshape(N, D)
    dk = torch.einsum('nhj,nhd->njhd', dl, qh).reshape(N, 2, D)
    dv = torch.einsum('nhj,nhd->njhd', a, doh).reshape(N, 2, D)
    return dq, torch.cat([dk, dv], -1)


def softmax_bwd(g, d):
    """d logits of softmax weights g for upstream d."""
    return g * (d - (g * d).sum(-1, keepdim=True))


# ---------------------------------------------------------------- stage lists
AUX_NAMES = ('opnd.', 'tol.', 'pert.', 'pre')     # what a stage returns besides its stored outputs


def run_chain(stages, bufs):
    """Every stage fed by the ones before it: the whole operation.  Returns bufs (updated)."""
    for _, fn in stages:
        bufs.update(fn(bufs))
    return bufs


def stage_pairs(stages, bufs):
    """Every stage fed by `bufs`' own stored inputs: yields (stage, name, stored, recomputed) for
    each output the stage produces that `bufs` holds."""
    for stage, fn in stages:
        for name, ref in fn(bufs).items():
            if name in bufs and not name.startswith(AUX_NAMES):
                yield stage, name, bufs[name], ref


def rel_err(got, ref):
    """max |got - ref| relative to max |ref| (0 / 0 -> 0)."""
    got, ref = torch.as_tensor(got).to(F64), torch.as_tensor(ref).to(F64)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    if scale == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return err / scale


# ================================================================ the DAMA frame head
HN, HD = 64, 128


def head_layout():
    """(name, offset, shape) of every buffer of csrc/head.hip's `struct HeadWs`, in floats, and
    the total including the 256-float trace tail."""
    out, o = [], 0

    def put(name, *shape):
        nonlocal o
        n = 1
        for s in shape:
            n *= s
        out.append((name, o, shape))
        o += n
    for i in range(6):
        put(f'st{i}', HN, HD)
    for i in range(4):
        put(f'xn{i}', HN, HD)
        put(f'mu{i}', HN)
        put(f'rs{i}', HN)
        put(f'q{i}', HN, HD)
        put(f'kv{i}', HN, 2, 2 * HD)
        put(f'at{i}', HN, 4, 2)
        put(f'o{i}', HN, HD)
    put('yfg', HN, HD)
    put('bnm', HD)
    put('bni', HD)
    put('fus', HN, HD)
    put('h1', HN, 64)
    put('gw', HN, 4)
    for i in range(4):
        put(f'dxn{i}', HN, HD)
        put(f'dq{i}', HN, HD)
        put(f'dkv{i}', HN, 2, 2 * HD)
        put(f'dpre{i}', HN, HD)
    put('dy', HN, HD)
    put('dh1', HN, 64)
    put('dz2', HN, 4)
    put('ds_s', HN, HD)
    put('ds_f', HN, HD)
    put('wc', HD, 256)          # unused by the kernels; kept for the layout
    return out, o + 256


def head_ws_views(ws, workspace_bytes, N=None):
    """{name: tensor} over the float32 workspace `ws` of ewvit_head_fwd / ewvit_head_bwd;
    `workspace_bytes` is what ewvit_head_workspace() reports.  N: keep the first N frames."""
    lay, total = head_layout()
    assert total * 4 == int(workspace_bytes), (total * 4, int(workspace_bytes))
    assert ws.dtype == torch.float32 and ws.numel() == total, (ws.dtype, ws.numel(), total)
    views = {}
    for name, o, shape in lay:
        n = 1
        for s in shape:
            n *= s
        v = ws[o:o + n].view(*shape)
        if N is not None and shape[0] == HN and name != 'wc':
            v = v[:N]
        views[name] = v
    return views


def head_param_list(cross_att, fusion_gate, gate_net):
    """The head's 32 parameters in the kernel's order (ewvit.head.params_of), from any modules
    with the reference's structure (oracle or product)."""
    ts = []
    for layer in cross_att.layers:
        for norm, att in ((layer[0], layer[1]), (layer[2], layer[3])):
            ts += [norm.weight, norm.bias, att.to_q.weight, att.to_kv.weight, att.to_out[0].weight, att.to_out[0].bias]
    ts += [fusion_gate[0].weight, fusion_gate[0].bias, fusion_gate[1].weight, fusion_gate[1].bias,
           gate_net[2].weight, gate_net[2].bias, gate_net[5].weight, gate_net[5].bias]
    return ts


HEAD_PARAM_NAMES = [f'ca{i}.{n}' for i in range(4) for n in ('ln_w', 'ln_b', 'wq', 'wkv', 'wo', 'bo')] + \
    ['wfg', 'bfg', 'bn_w', 'bn_b', 'g1w', 'g1b', 'g2w', 'g2b']


def head_params(ts):
    """{name: float64 CPU tensor} of the 32 parameters (HEAD_PARAM_NAMES order)."""
    assert len(ts) == 32
    return {n: t.detach().to('cpu', F64) for n, t in zip(HEAD_PARAM_NAMES, ts)}


# block i reads state st[xin], context st[cin], writes st[xout] (0 = layer 0 s, 1 = layer 0 f, ...)
def h_xin(i):
    return (i >> 1) * 2 + (i & 1)


def h_xout(i):
    return (i >> 1) * 2 + 2 + (i & 1)


def h_cin(i):
    return (i >> 1) * 2 + 2 if i & 1 else (i >> 1) * 2 + 1


class HeadCfg:
    """What a head call fixes besides its tensors.  masks: {0..3: [N, 128], 4: [N, 64]}, each
    element 0 or 1 / (1 - p); rounding: of the attention blocks' GEMMs (the fusion conv and the
    gate's first layer are bf16 in both of the kernel's forms, exact when rounding is None);
    bn: (running_mean, running_var, num_batches_tracked, momentum, eps) before the call."""

    def __init__(self, P, masks, rounding, training, bn, ln_eps=1e-5):
        self.P, self.masks, self.rounding, self.training, self.ln_eps = P, masks, rounding, training, ln_eps
        self.rm, self.rv, self.nbt, self.mom, self.bn_eps = bn
        self.r2 = None if rounding is None else 'bf16'


def _concat(b):
    return torch.cat([b['st4'], b['st5']], 1)


def head_fwd_stages(c):
    """The forward of csrc/head.hip stage by stage (dama.py:143-169)."""
    P, st = c.P, []

    def block(i):
        xin, xout, cin = f'st{h_xin(i)}', f'st{h_xout(i)}', f'st{h_cin(i)}'

        def ln(b):
            y, mu, rs = layernorm(b[xin], P[f'ca{i}.ln_w'], P[f'ca{i}.ln_b'], c.ln_eps)
            return {f'xn{i}': y, f'mu{i}': mu, f'rs{i}': rs}

        def qkv(b):                       # to_q of the normed token, to_kv of (normed self, context)
            kv = torch.stack([linear(b[f'xn{i}'], P[f'ca{i}.wkv'], c.rounding),
                              linear(b[cin], P[f'ca{i}.wkv'], c.rounding)], 1)
            return {f'q{i}': linear(b[f'xn{i}'], P[f'ca{i}.wq'], c.rounding), f'kv{i}': kv}

        def att(b):
            a, o = attn_1x2(b[f'q{i}'], b[f'kv{i}'])
            return {f'at{i}': a, f'o{i}': o}

        def out(b):                       # to_out + bias, dropout, residual (dama.py:50-53, 71-76)
            pre = linear(b[f'o{i}'], P[f'ca{i}.wo'], c.rounding) + P[f'ca{i}.bo']
            return {xout: b[xin] + pre * c.masks[i], f'pre{i}': pre}
        return [(f'ln{i}', ln), (f'qkv{i}', qkv), (f'att{i}', att), (f'out{i}', out)]
    for i in range(4):
        st += block(i)

    def fuse(b):                          # the centre tap of Conv3x3 on the 1x1 map; gate Linear 1
        cat = _concat(b)
        return {'yfg': linear(cat, P['wfg'][:, :, 1, 1], c.r2), 'h1': linear(cat, P['g1w'], c.r2)}

    def bn(b):
        y = b['yfg'] + P['bfg']
        N = y.shape[0]
        if c.training:
            m = y.mean(0)
            q = ((y - m) ** 2).sum(0)
            var, unb = q / N, q / max(N - 1, 1)
            out = {'bn_rm': (1 - c.mom) * c.rm + c.mom * m, 'bn_rv': (1 - c.mom) * c.rv + c.mom * unb,
                   'bn_nbt': c.nbt + 1}
        else:
            m, var = c.rm, c.rv
            out = {'bn_rm': c.rm, 'bn_rv': c.rv, 'bn_nbt': c.nbt}
        iv = 1.0 / torch.sqrt(var + c.bn_eps)
        out.update({'bnm': m, 'bni': iv, 'fus': torch.relu((y - m) * iv * P['bn_w'] + P['bn_b'])})
        return out

    def gate(b):                          # ReLU, dropout, Linear 2, softmax (dama.py:105-113)
        hd = torch.relu(b['h1'] + P['g1b']) * c.masks[4]
        g = torch.softmax(hd @ P['g2w'].t() + P['g2b'], -1)
        return {'gw': torch.cat([g, g.new_zeros(g.shape[0], 1)], 1)}

    def wsum(b):                          # dama.py:159-163
        g = b['gw']
        return {'fused': g[:, 0:1] * b['st4'] + g[:, 1:2] * b['st5'] + g[:, 2:3] * b['fus'],
                's_out': b['st4'], 'f_out': b['st5']}
    return st + [('fuse', fuse), ('bn', bn), ('gate', gate), ('sum', wsum)]


def _head_streams(c, b, upto):
    """The two streams' gradients (d s, d f) as head_bwd_rows_kernel holds them BEFORE block
    `upto` (3, 2, 1, 0; -1: after block 0 = d s0, d f0), from the stored buffers: the tail's
    ds_s / ds_f, the fusion conv / gate input gradient of (dy, dh1), and per finished block its
    LayerNorm backward of dxn (own stream) and to_kv's input gradient of dkv[:, 1] (context)."""
    P = c.P
    dcat = dgrad(b['dy'], P['wfg'][:, :, 1, 1], c.r2) + dgrad(b['dh1'], P['g1w'], c.r2)
    d = [b['ds_s'] + dcat[:, :HD], b['ds_f'] + dcat[:, HD:]]
    for i in range(3, upto, -1):
        own, ctx = i & 1, 1 - (i & 1)
        d[ctx] = d[ctx] + dgrad(b[f'dkv{i}'][:, 1], P[f'ca{i}.wkv'], c.rounding)
        d[own] = d[own] + layernorm_bwd(b[f'dxn{i}'], b[f'st{h_xin(i)}'], b[f'mu{i}'], b[f'rs{i}'], P[f'ca{i}.ln_w'])[0]
    return d


def head_bwd_stages(c):
    """The backward of csrc/head.hip stage by stage; inputs g_fused, g_s, g_f under those names.
    Parameter gradients come out as 'g.<HEAD_PARAM_NAMES entry>'."""
    P, st = c.P, []

    def tail_sum(b):
        g = b['gw']
        return {'ds_s': b['g_s'] + g[:, 0:1] * b['g_fused'], 'ds_f': b['g_f'] + g[:, 1:2] * b['g_fused']}

    def tail_gate(b):
        gf = b['g_fused']
        d = torch.stack([(gf * b['st4']).sum(1), (gf * b['st5']).sum(1), (gf * b['fus']).sum(1)], 1)
        dz = softmax_bwd(b['gw'][:, :3], d)
        return {'dz2': torch.cat([dz, dz.new_zeros(dz.shape[0], 1)], 1)}

    def tail_dh1(b):                      # d pre-activation = (dz2 W2) * dropout * relu'
        live = (b['h1'] + P['g1b']) > 0
        return {'dh1': (b['dz2'][:, :3] @ P['g2w']) * c.masks[4] * live}

    def tail_bn(b):                       # ReLU + BatchNorm backward over the frames
        N = b['yfg'].shape[0]
        gr = b['g_fused'] * b['gw'][:, 2:3] * (b['fus'] > 0)
        xh = (b['yfg'] + P['bfg'] - b['bnm']) * b['bni']
        SG, SGX = gr.sum(0), (gr * xh).sum(0)
        k = P['bn_w'] * b['bni']
        dy = k * (gr - SG / N - xh * SGX / N) if c.training else k * gr
        return {'dy': dy, 'g.bn_w': SGX, 'g.bn_b': SG}
    st += [('tail_sum', tail_sum), ('tail_gate', tail_gate), ('tail_dh1', tail_dh1), ('tail_bn', tail_bn)]

    def block(i):
        def dpre(b):                      # to_out's dropout on the own stream's gradient
            return {f'dpre{i}': _head_streams(c, b, i)[i & 1] * c.masks[i]}

        def dattn(b):                     # d o = dpre Wo (not stored), then the attention backward
            do = dgrad(b[f'dpre{i}'], P[f'ca{i}.wo'], c.rounding)
            dq, dkv = attn_1x2_bwd(do, b[f'q{i}'], b[f'kv{i}'], b[f'at{i}'])
            return {f'dq{i}': dq, f'dkv{i}': dkv}

        def dxn(b):                       # d LN output = dq Wq + dkv_self Wkv
            return {f'dxn{i}': dgrad(b[f'dq{i}'], P[f'ca{i}.wq'], c.rounding) +
                    dgrad(b[f'dkv{i}'][:, 0], P[f'ca{i}.wkv'], c.rounding)}
        return [(f'dpre{i}', dpre), (f'dattn{i}', dattn), (f'dxn{i}', dxn)]
    for i in (3, 2, 1, 0):
        st += block(i)

    def dinputs(b):
        d = _head_streams(c, b, -1)
        return {'ds0': d[0], 'df0': d[1]}

    def weights(b):
        g, cat = {}, _concat(b)
        for i in range(4):
            xn, ctx = b[f'xn{i}'], b[f'st{h_cin(i)}']
            dkv = b[f'dkv{i}']
            g[f'g.ca{i}.wq'] = wgrad(b[f'dq{i}'], xn, c.rounding, HN)
            g[f'g.ca{i}.wkv'] = wgrad(dkv[:, 0], xn, c.rounding, HN) + wgrad(dkv[:, 1], ctx, c.rounding, HN)
            g[f'g.ca{i}.wo'] = wgrad(b[f'dpre{i}'], b[f'o{i}'], c.rounding, HN)
            g[f'g.ca{i}.bo'] = b[f'dpre{i}'].sum(0)
            _, g[f'g.ca{i}.ln_w'], g[f'g.ca{i}.ln_b'] = layernorm_bwd(
                b[f'dxn{i}'], b[f'st{h_xin(i)}'], b[f'mu{i}'], b[f'rs{i}'], P[f'ca{i}.ln_w'])
        wfg = torch.zeros_like(P['wfg'])              # the 8 taps that only ever meet padding: 0
        wfg[:, :, 1, 1] = wgrad(b['dy'], cat, c.r2)
        hd = torch.relu(b['h1'] + P['g1b']) * c.masks[4]
        g.update({'g.wfg': wfg, 'g.bfg': b['dy'].sum(0), 'g.g1w': wgrad(b['dh1'], cat, c.r2),
                  'g.g1b': b['dh1'].sum(0), 'g.g2w': b['dz2'][:, :3].t() @ hd, 'g.g2b': b['dz2'][:, :3].sum(0)})
        return g
    return st + [('dinputs', dinputs), ('weights', weights)]


# ---------------------------------------------------------------- mask recovery (head)
def recover_ca_mask(st_in, st_out, pre, p, floor=1e-4):
    """The to_out dropout mask of one attention block from what the forward stored: an element
    was kept iff st_out != st_in.  `pre` is the float64 pre-dropout value o Wo^T + bo; where
    |pre| < floor of its scale the comparison says nothing when the two are equal (a kept tiny
    value may vanish in the fp32 add): such elements are unreadable and count as kept.
    -> (mask scaled by 1 / (1 - p), kept [bool], unreadable [bool])."""
    changed = st_out != st_in
    small = pre.abs() < floor * float(pre.abs().max())
    unreadable = small & ~changed
    kept = changed | unreadable
    return kept.to(F64) / (1.0 - p), kept, unreadable, small


def recover_gate_mask(dh1, dz2, h1, g1b, g2w, p, tol=1e-4, floor=1e-4):
    """The gate dropout mask from what the backward stored: on ReLU-live units dh1 / (dz2 W2) is
    0 for a dropped unit and 1 / (1 - p) for a kept one.  ReLU-dead units carry no mask
    information and influence nothing (kept); live units with |dz2 W2| < floor of scale are
    unreadable (kept).  -> (scaled mask, kept, live, unreadable, ok) with ok False when a readable
    live unit's ratio is neither value within tol."""
    live = (h1 + g1b) > 0
    den = dz2[:, :3] @ g2w
    small = den.abs() < floor * float(den.abs().max())
    readable = live & ~small
    ratio = torch.where(readable, dh1 / torch.where(readable, den, torch.ones_like(den)), torch.zeros_like(den))
    is_drop = readable & (ratio.abs() <= tol)
    is_keep = readable & ((ratio - 1.0 / (1.0 - p)).abs() <= tol)
    ok = bool((is_drop | is_keep)[readable].all())
    kept = ~is_drop
    return kept.to(F64) / (1.0 - p), kept, live, live & small, ok


def head_inputs(N):
    """The head tests' inputs at N frames (CPU fp32, fixed seeds): the two branch tokens and the
    three upstream gradients."""
    g = torch.Generator().manual_seed(1000 + N)
    s0 = torch.randn(N, HD, generator=g) * 2
    f0 = torch.randn(N, HD, generator=g)
    return s0, f0, [torch.randn(N, HD, generator=g) for _ in range(3)]


def resolve_gate_unreadable(mask, unreadable, h1, g1b, g2w, g2b, gw, p):
    """The few live gate units the backward cannot read (`recover_gate_mask`), settled from the
    forward instead: of kept / dropped, the value under which the frame's logits reproduce the
    stored softmax weights better.  Returns the mask with those units set."""
    mask = mask.clone()
    for n, j in unreadable.nonzero().tolist():
        best = None
        for val in (1.0 / (1.0 - p), 0.0):
            mask[n, j] = val
            g = torch.softmax((torch.relu(h1[n] + g1b) * mask[n]) @ g2w.t() + g2b, -1)
            err = float((g - gw[n, :3]).abs().max())
            if best is None or err < best[0]:
                best = (err, val)
        mask[n, j] = best[1]
    return mask


# ================================================================ the ViT encoder layer
VD, VQ, VF, VH, VDH, VRP = 512, 1536, 2048, 8, 64, 128
VIT_PARAM_NAMES = ['ln1_w', 'ln1_b', 'wqkv', 'wo', 'bo', 'ln2_w', 'ln2_b', 'w1', 'b1', 'w2', 'b2']

_SAVED = [('mu1', 'f', (VRP,)), ('rs1', 'f', (VRP,)), ('mu2', 'f', (VRP,)), ('rs2', 'f', (VRP,)),
          ('p', 'f', (VRP, VH, 2)), ('x1', 'f', (VRP, VD)), ('qkv', 'b', (VRP, VQ)), ('aux', 'b', (VRP, VF)),
          ('h', 'b', (VRP, VF)), ('ln1T', 'b', (VD, VRP)), ('oT', 'b', (VD, VRP)), ('ln2T', 'b', (VD, VRP)),
          ('hT', 'b', (VF, VRP)), ('ws2', 'f', (16, VRP, VD))]
_SCRATCH = [('gT', 'b', (VD, VRP)), ('g1', 'b', (VRP, VF)), ('g1T', 'b', (VF, VRP)), ('goT', 'b', (VD, VRP)),
            ('dqkv', 'b', (VRP, VQ)), ('dqkvT', 'b', (VQ, VRP)), ('dln2', 'f', (VRP, VD)), ('dx1', 'f', (VRP, VD)),
            ('dln1', 'f', (VRP, VD)), ('rp2', 'f', (32, VRP, 2)), ('rp1', 'f', (32, VRP, 2)), ('db1p', 'f', (2, VF))]


def _blob_views(blob, layout, expect_bytes):
    """Named views of a uint8 blob laid out as csrc/vit.hip's saved_layout / scratch_layout: the
    buffers in order, each padded to 256 bytes ('f' float32, 'b' bfloat16)."""
    assert blob.dtype == torch.uint8 and blob.dim() == 1
    views, o = {}, 0
    for name, kind, shape in layout:
        n = 1
        for s in shape:
            n *= s
        nb = n * (4 if kind == 'f' else 2)
        views[name] = blob[o:o + nb].view(torch.float32 if kind == 'f' else torch.bfloat16).view(*shape)
        o += (nb + 255) // 256 * 256
    assert o == int(expect_bytes) == blob.numel(), (o, int(expect_bytes), blob.numel())
    return views


def vit_saved_views(blob, workspace_bytes):
    """`saved` of ewvit_vit_layer_fwd; workspace_bytes = ewvit_vit_layer_workspace(0)."""
    return _blob_views(blob, _SAVED, workspace_bytes)


def vit_scratch_views(blob, workspace_bytes):
    """`scratch` of ewvit_vit_layer_bwd; workspace_bytes = ewvit_vit_layer_workspace(1)."""
    return _blob_views(blob, _SCRATCH, workspace_bytes)


def vit_layout_bytes():
    def total(layout):
        o = 0
        for _, kind, shape in layout:
            n = 1
            for s in shape:
                n *= s
            o += (n * (4 if kind == 'f' else 2) + 255) // 256 * 256
        return o
    return total(_SAVED), total(_SCRATCH)


def vit_param_list(attn, ff):
    """The layer's 11 parameters in the kernel's order (ewvit.vit.params_of) from a
    (PreNorm(Attention), PreNorm(FeedForward)) pair of the oracle or the product."""
    a, f = attn.fn, ff.fn
    return [attn.norm.weight, attn.norm.bias, a.to_qkv.weight, a.to_out[0].weight, a.to_out[0].bias,
            ff.norm.weight, ff.norm.bias, f.net[0].weight, f.net[0].bias, f.net[3].weight, f.net[3].bias]


def vit_params(ts):
    assert len(ts) == 11
    return {n: t.detach().to('cpu', F64) for n, t in zip(VIT_PARAM_NAMES, ts)}


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def gelu_erf_grad(x):
    return 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) * (2.0 * torch.pi) ** -0.5


def attn_2x2(qkv, heads=VH):
    """sfe.py:42-70 on two tokens per frame (rows 2b, 2b + 1): -> softmax weights
    p[row][head][key] and the merged attention output [R, 512]."""
    R, D = qkv.shape[0], qkv.shape[1] // 3
    q, k, v = (t.reshape(R // 2, 2, heads, D // heads) for t in qkv.split(D, -1))
    a = torch.softmax(torch.einsum('bihd,bjhd->bhij', q, k) * (D // heads) ** -0.5, -1)
    o = torch.einsum('bhij,bjhd->bihd', a, v).reshape(R, D)
    return a.permute(0, 2, 1, 3).reshape(R, heads, 2), o


def attn_2x2_bwd(do, qkv, p, heads=VH):
    R, D = qkv.shape[0], qkv.shape[1] // 3
    dh = D // heads
    q, k, v = (t.reshape(R // 2, 2, heads, dh) for t in qkv.split(D, -1))
    a = p.reshape(R // 2, 2, heads, 2).permute(0, 2, 1, 3)             # [b, h, i, j]
    doh = do.reshape(R // 2, 2, heads, dh)
    da = torch.einsum('bihd,bjhd->bhij', doh, v)
    ds = a * (da - (a * da).sum(-1, keepdim=True)) * dh ** -0.5
    dq = torch.einsum('bhij,bjhd->bihd', ds, k).reshape(R, D)
    dk = torch.einsum('bhij,bihd->bjhd', ds, q).reshape(R, D)
    dv = torch.einsum('bhij,bihd->bjhd', a, doh).reshape(R, D)
    return torch.cat([dq, dk, dv], -1)


def attn_2x2_bwd_abs(pert, qkv, p, heads=VH):
    """First-order bound on what a perturbation |delta do| <= pert (elementwise) of the attention
    output's gradient does to attn_2x2_bwd's result: the same sums over absolute values."""
    R, D = qkv.shape[0], qkv.shape[1] // 3
    dh = D // heads
    q, k, v = (t.abs().reshape(R // 2, 2, heads, dh) for t in qkv.split(D, -1))
    a = p.reshape(R // 2, 2, heads, 2).permute(0, 2, 1, 3)
    ph = pert.reshape(R // 2, 2, heads, dh)
    eda = torch.einsum('bihd,bjhd->bhij', ph, v)
    eds = a * (eda + (a * eda).sum(-1, keepdim=True)) * dh ** -0.5
    edq = torch.einsum('bhij,bjhd->bihd', eds, k).reshape(R, D)
    edk = torch.einsum('bhij,bihd->bjhd', eds, q).reshape(R, D)
    edv = torch.einsum('bhij,bihd->bjhd', a, ph).reshape(R, D)
    return torch.cat([edq, edk, edv], -1)


def bf16_mid_pert(x):
    """How far a value the kernel rounds to bf16 WITHOUT storing it may sit from its float64
    reference x: one round-to-nearest (2^-8 relative) of a value itself within the fp32 bound
    (1e-4 of scale)."""
    return 2.0 ** -8 * x.abs() + 1e-4 * float(x.abs().max())


class VitCfg:
    """mask: the to_out dropout [R, 512], elements 0 or 1 / (1 - p)."""

    def __init__(self, P, mask, rounding, ln_eps=1e-5):
        self.P, self.mask, self.rounding, self.ln_eps = P, mask, rounding, ln_eps
        self.override = {}      # {output name: the already quantized A operand to use} (resolve_rows)

    def mm(self, key, a, Wk):
        """a [R, K] times Wk [O, K]^T for the stages whose MX operand the kernel quantizes from
        fp32 values it does not store."""
        aq = self.override.get(key)
        if aq is None:
            aq = _opnd(a, self.rounding, False)
        return aq @ _opnd(Wk, self.rounding, False).t()


def vit_fwd_stages(c):
    """csrc/vit.hip forward (sfe.py:72-85).  Buffers the kernel keeps transposed are named by
    their row-major content here: ln1 = ln1T^T, o = oT^T, ln2 = ln2T^T.  In MXFP8 form the kernel
    quantizes the LayerNorm outputs and the attention output from fp32 values it does not store:
    those operands ('opnd.<output>') are recomputed from the stage's stored inputs (x0 / x1 with
    the stored statistics; p and qkv), with 'tol.<output>', a bound on how far the kernel's fp32
    evaluation of the same expression may sit from them."""
    P, mx = c.P, c.rounding == 'mx'

    def ln1(b):
        y, mu, rs = layernorm(b['x0'], P['ln1_w'], P['ln1_b'], c.ln_eps)
        return {'ln1': y, 'mu1': mu, 'rs1': rs}

    def qkv(b):
        a, tol = b['ln1'], None
        if mx:                            # from the stored statistics, as the kernel's fragments form it
            t = (b['x0'] - b['mu1'][:, None]) * b['rs1'][:, None] * P['ln1_w']
            a, tol = t + P['ln1_b'], 2.0 ** -21 * (t.abs() + P['ln1_b'].abs())
        return {'qkv': c.mm('qkv', a, P['wqkv']), 'opnd.qkv': a, 'tol.qkv': tol}

    def att(b):
        p, o = attn_2x2(b['qkv'])
        return {'p': p, 'o': o}

    def out(b):
        a, tol = b['o'], None
        if mx:                            # from the stored softmax weights and the stored v
            R = b['qkv'].shape[0]
            v = b['qkv'][:, 2 * VD:].reshape(R // 2, 2, VH, VDH)
            pp = b['p'].reshape(R // 2, 2, VH, 2)
            a = torch.einsum('bihj,bjhd->bihd', pp, v).reshape(R, VD)
            tol = 2.0 ** -22 * torch.einsum('bihj,bjhd->bihd', pp, v.abs()).reshape(R, VD)
        pre = c.mm('x1', a, P['wo']) + P['bo']
        return {'x1': b['x0'] + pre * c.mask, 'pre1': pre, 'opnd.x1': a, 'tol.x1': tol}

    def ln2(b):
        y, mu, rs = layernorm(b['x1'], P['ln2_w'], P['ln2_b'], c.ln_eps)
        return {'ln2': y, 'mu2': mu, 'rs2': rs}

    def mlp1(b):
        a, tol = b['ln2'], None
        if mx:
            t = (b['x1'] - b['mu2'][:, None]) * b['rs2'][:, None] * P['ln2_w']
            a, tol = t + P['ln2_b'], 2.0 ** -21 * (t.abs() + P['ln2_b'].abs())
        pre = c.mm('aux', a, P['w1']) + P['b1']
        return {'aux': pre, 'h': gelu_erf(pre), 'opnd.aux': a, 'tol.aux': tol}

    def mlp2(b):
        return {'x2': b['x1'] + linear(b['h'], P['w2'], c.rounding) + P['b2']}
    return [('ln1', ln1), ('qkv', qkv), ('att', att), ('out', out), ('ln2', ln2), ('mlp1', mlp1), ('mlp2', mlp2)]


def vit_bwd_stages(c):
    """csrc/vit.hip backward; upstream gradient under 'g'.  go = goT^T (to_out's output gradient
    after the dropout).  'opnd.<name>' / 'tol.<name>' as in the forward.  dh = g W2 and d(attention
    out) = g_o Wo are rounded to bf16 without being stored: the references keep them unrounded and
    'pert.<name>' bounds what that rounding may add to the stage's output (`bf16_mid_pert`)."""
    P, mx = c.P, c.rounding == 'mx'

    def mlp2_bwd(b):                      # dh = g W2 rounded to bf16, g1 = dh GELU'(pre)
        dh = dgrad(b['g'], P['w2'], c.rounding, False)
        dg = gelu_erf_grad(b['aux'])
        g1 = dh * dg
        return {'g1': g1, 'g.b2': b['g'].sum(0), 'g.b1': g1.sum(0), 'pert.g1': bf16_mid_pert(dh) * dg.abs()}

    def mlp1_bwd(b):
        gt = b['g'] if c.rounding is None else bf16(b['g'])          # gT holds g as bf16
        return {'dln2': dgrad(b['g1'], P['w1'], c.rounding), 'g.w2': wgrad(gt, b['h'], c.rounding),
                'g.w1': wgrad(b['g1'], b['ln2'], c.rounding)}

    def ln2_bwd(b):
        dx, dw, db = layernorm_bwd(b['dln2'], b['x1'], b['mu2'], b['rs2'], P['ln2_w'])
        return {'dx1': dx + b['g'], 'g.ln2_w': dw, 'g.ln2_b': db}

    def drop_bwd(b):
        go = b['dx1'] * c.mask
        return {'go': go, 'g.bo': go.sum(0)}

    def attn_bwd(b):
        a, tol = b['go'], None
        if mx:                            # g_o from the stored dx1: the fragments evaluate the LN2 backward again
            a = b['dx1'] * c.mask
            t = layernorm_bwd(b['dln2'], b['x1'], b['mu2'], b['rs2'], P['ln2_w'].abs())[0].abs()
            u = (b['rs2'][:, None] * P['ln2_w'] * b['dln2']).abs()
            tol = 2.0 ** -20 * (b['dx1'].abs() + b['g'].abs() + t + u) * c.mask
        do = c.mm('dqkv', a, P['wo'].t())
        return {'dqkv': attn_2x2_bwd(do, b['qkv'], b['p']), 'opnd.dqkv': a, 'tol.dqkv': tol,
                'pert.dqkv': attn_2x2_bwd_abs(bf16_mid_pert(do), b['qkv'], b['p'])}

    def qkv_bwd(b):
        return {'dln1': dgrad(b['dqkv'], P['wqkv'], c.rounding), 'g.wqkv': wgrad(b['dqkv'], b['ln1'], c.rounding),
                'g.wo': wgrad(b['go'], b['o'], c.rounding)}

    def ln1_bwd(b):
        dx, dw, db = layernorm_bwd(b['dln1'], b['x0'], b['mu1'], b['rs1'], P['ln1_w'])
        return {'dx0': dx + b['dx1'], 'g.ln1_w': dw, 'g.ln1_b': db}
    return [('mlp2_bwd', mlp2_bwd), ('mlp1_bwd', mlp1_bwd), ('ln2_bwd', ln2_bwd), ('drop_bwd', drop_bwd),
            ('attn_bwd', attn_bwd), ('qkv_bwd', qkv_bwd), ('ln1_bwd', ln1_bwd)]


def ln_row_partials(d, x, mu, rs, gamma):
    """The LayerNorm-backward row partials the input-gradient kernels leave per 16-column block:
    [32][R][2] = (sum gamma d, sum gamma d xhat) over the block's columns."""
    xh = (x - mu[:, None]) * rs[:, None]
    ga = (gamma * d).view(d.shape[0], 32, 16).sum(-1).t()
    gb = (gamma * d * xh).view(d.shape[0], 32, 16).sum(-1).t()
    return torch.stack([ga, gb], -1)


def mx_alternatives(x, rel=2.0 ** -18, max_per_row=4, abs_tol=None):
    """MXFP8 of x [R, K] with its doubtful roundings spelled out: -> (q, alts, left_out).  q is the
    default quantization (`mxq`); alts {row: [(k, delta)]} lists the elements within `rel`
    (relative; or abs_tol, elementwise absolute, where that is wider) of an e4m3 rounding
    boundary with what the other rounding would add to q[row, k]; left_out marks
    the rows that cannot be settled that way (a block maximum within `rel` of the boundary that
    selects the block scale, or more than max_per_row doubtful elements)."""
    R, K = x.shape
    q = mxq(x)
    xb = x.abs().view(R, K // 32, 32)
    amax = xb.amax(-1)
    m, e = torch.frexp(amax)
    near_scale = ((2 * m - 1.75).abs() <= 1.75 * rel) & (amax > 0)
    X = torch.where(amax > 0, e - 1 - 8 + (2 * m > 1.75).int(), torch.zeros_like(e))
    s = torch.pow(2.0, X.to(F64)).unsqueeze(-1)
    y = xb / s
    sp = torch.pow(2.0, torch.floor(torch.log2(y.clamp_min(2.0 ** -6))) - 3)
    lower = torch.floor(y / sp) * sp
    win = rel * y if abs_tol is None else torch.maximum(rel * y, abs_tol.view(R, K // 32, 32) / s)
    near = (((y - lower) / sp - 0.5).abs() * sp <= win) & (y > 0)
    if abs_tol is not None:
        near_scale = near_scale | ((amax - 1.75 * torch.pow(2.0, (e - 1).to(F64))).abs()
                                   <= abs_tol.view(R, K // 32, 32).amax(-1))
    qy = q.abs().view(R, K // 32, 32) / s
    alt = torch.where(qy > lower, lower, lower + sp)
    delta = ((alt - qy) * s * torch.sign(x.view(R, K // 32, 32))).view(R, K)
    near = near.view(R, K)
    alts = {}
    for r, k in near.nonzero().tolist():
        alts.setdefault(r, []).append((k, float(delta[r, k])))
    left = near_scale.any(-1) | (near.sum(-1) > max_per_row)
    return q, alts, left


def resolve_rows(q, alts, left, Wq, post, got):
    """Settle the doubtful roundings of `mx_alternatives` against what the kernel stored: for each
    row the combination of alternatives whose output post(row, q_row Wq^T) is closest to got(row) in
    the least-squares sense (the other rounding of element k moves the row along Wq[:, k]; the
    rounding of a bf16-stored row is noise across it).
    Wq [O, K]: the other operand, already quantized.  Returns q with the chosen alternatives."""
    q = q.clone()
    for r, cand in alts.items():
        if bool(left[r]):
            continue
        base = q[r] @ Wq.t()
        best = None
        for pick in range(1 << len(cand)):
            out = base.clone()
            for j, (k, d) in enumerate(cand):
                if pick >> j & 1:
                    out = out + d * Wq[:, k]
            cost = float(((post(r, out) - got(r)) ** 2).sum())
            if best is None or cost < best[0]:
                best = (cost, pick)
        for j, (k, d) in enumerate(cand):
            if best[1] >> j & 1:
                q[r, k] += d
    return q


def vit_inputs(B):
    """The ViT stage tests' input tokens [B, 2, 512] and upstream gradient (CPU fp32, fixed seeds)."""
    g = torch.Generator().manual_seed(2000 + B)
    return torch.randn(B, 2, VD, generator=g), torch.randn(B, 2, VD, generator=g)

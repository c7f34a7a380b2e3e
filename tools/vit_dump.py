"""Everything csrc/vit.hip and the tall-K GEMM write, into one .npz, for a bit comparison of two
builds of the library (EWVIT_LIB selects the one under test): a restructuring of those kernels
must leave every array byte-equal — they sum in fixed orders and the dropout mask is a pure
function of seed and counter.

Calls the C ABI directly with zero-filled saved / scratch / output / gradient buffers (the
autograd functions allocate with torch.empty, whose unwritten bytes cannot be compared), on the
stage tests' layer and inputs: 64 / 37 / 1 frames x bf16 / MXFP8 x to_out dropout 0.15 / 0.0, both
weight packs, the token embedding forward / backward at 13 frames and ewvit_gemm_tallk at
M = 37, N = 256, K = 512 (the smallest shape of its class with a ragged row tile).
Usage: python tools/vit_dump.py OUT.npz      compare: python tools/vit_dump.py --cmp A.npz B.npz"""
import copy
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'efficient-wavelet-vit_amd'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
DEV = 'cuda'


def _bytes(t):
    return t.detach().contiguous().view(torch.uint8).cpu().numpy()


def _zeros(n):
    return torch.zeros(int(n), dtype=torch.uint8, device=DEV)


def _pack(L, ev, layer, mx):
    buf = _zeros(ev._ws_bytes(3 if mx else 2))
    arr = (ev._Params * 1)()
    arr[0] = ev._params(ev.params_of(*layer), 0.0, 0.0, 0, torch.device(DEV))
    L.call('ewvit_vit_pack_mx' if mx else 'ewvit_vit_pack', ctypes.addressof(arr), 1, L.ptr(buf), L.stream(buf))
    return buf


def _layer(out, L, ev, fr, m, B, mx, drop):
    layer = copy.deepcopy(m).layers[0]
    ts = [t.detach() for t in ev.params_of(*layer)]
    R = 2 * B
    xc, gc = fr.vit_inputs(B)
    x0, g = xc.to(DEV).reshape(R, 512).contiguous(), gc.to(DEV).reshape(R, 512).contiguous()
    dev = x0.device
    L.rng_offset(dev).zero_()            # the stage tests' step counter
    L.rng_advance(dev)
    buf = _pack(L, ev, layer, mx)
    saved, scratch = _zeros(ev._ws_bytes(0)), _zeros(ev._ws_bytes(1))
    x2, dx0 = torch.zeros_like(x0), torch.zeros_like(x0)
    grads = [torch.zeros_like(t) for t in ts]
    p = ev._params(ts, layer[0].norm.eps, drop, 4242 if drop > 0 else 0, dev, buf.data_ptr(), mx)
    G = ev._Grads(*[o.data_ptr() for o in grads])
    L.call('ewvit_vit_layer_fwd', ctypes.addressof(p), R, L.ptr(x0), L.ptr(saved), L.ptr(x2), L.stream(x2))
    L.call('ewvit_vit_layer_bwd', ctypes.addressof(p), R, L.ptr(x0), L.ptr(saved), L.ptr(g), L.ptr(scratch),
           L.ptr(dx0), ctypes.addressof(G), L.stream(dx0))
    torch.cuda.synchronize()
    tag = f"B{B}_{'mx' if mx else 'bf16'}_p{drop}/"
    out[tag + 'pack'], out[tag + 'saved'], out[tag + 'scratch'] = _bytes(buf), _bytes(saved), _bytes(scratch)
    out[tag + 'x2'], out[tag + 'dx0'] = _bytes(x2), _bytes(dx0)
    for name, t in zip(fr.VIT_PARAM_NAMES, grads):
        out[tag + 'g.' + name] = _bytes(t)


def _embed(out, L, B=13, npos=64, drop=0.15, seed=4242):
    gen = torch.Generator().manual_seed(77)
    y, cls, pos, dtok = (torch.randn(*s, generator=gen).to(DEV) for s in ((B, 512), (512,), (npos, 512), (B, 2, 512)))
    dev = y.device
    L.rng_offset(dev).zero_()
    L.rng_advance(dev)
    off = L.rng_offset(dev)
    tok = torch.zeros(B, 2, 512, device=DEV)
    dy, dcls, dpos = torch.zeros_like(y), torch.zeros_like(cls), torch.zeros_like(pos)
    L.call('ewvit_vit_embed_fwd', L.ptr(y), L.ptr(cls), L.ptr(pos), B, npos, drop, seed, L.ptr(off), L.ptr(tok),
           L.stream(tok))
    L.call('ewvit_vit_embed_bwd', L.ptr(dtok), B, npos, drop, seed, L.ptr(off), L.ptr(dy), L.ptr(dcls), L.ptr(dpos),
           L.stream(dy))
    torch.cuda.synchronize()
    for k, t in (('tok', tok), ('dy', dy), ('dcls', dcls), ('dpos', dpos)):
        out['embed/' + k] = _bytes(t)


def _tallk(out, L, M=37, N=256, K=512):
    gen = torch.Generator().manual_seed(78)
    A = torch.randn(M, K, generator=gen).to(DEV).bfloat16()
    W, bias = torch.randn(N, K, generator=gen).to(DEV), torch.randn(N, generator=gen).to(DEV)
    C = torch.zeros(M, N, device=DEV)
    ws = _zeros(L.load().ewvit_gemm_tallk_workspace(M, N, K))
    L.call('ewvit_gemm_tallk', L.ptr(A), K, L.ptr(W), L.ptr(bias), L.ptr(C), N, M, N, K, L.ptr(ws), L.stream(C))
    torch.cuda.synchronize()
    out['tallk/C'], out['tallk/ws'] = _bytes(C), _bytes(ws)


def dump(path):
    import ewvit
    from ewvit import vit as ev
    import fused_ref as fr
    from test_gpu_vit import _vit
    L = ewvit._lib
    out = {}
    for drop in (0.15, 0.0):
        m = _vit(drop).train()
        for B in (64, 37, 1):
            for mx in (False, True):
                _layer(out, L, ev, fr, m, B, mx, drop)
    _embed(out, L)
    _tallk(out, L)
    np.savez(path, **out)
    print(f'vit_dump: {len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes, library {L.LIB_PATH} -> {path}')


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            n = int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else -1
            print(f'DIFFERS {k}: {n} of {a[k].size} bytes')
            bad.append(k)
    nz = sum(1 for k in a.files if a[k].any())
    print(f'vit_dump --cmp: {len(a.files)} arrays compared ({nz} non-zero), {len(bad)} differ')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--cmp':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])

"""Benchmark: DAMA fwd+bwd frames/s at 224x224, 64 frames per GPU, dim 128
(BASELINE.json configs[1]; configs[2] with --gpus N / torchrun on N GPUs).

One step = the reference training step of train.py:93-115 on synthetic data:
``DeepfakeDetector.forward(x[8, 8, 3, 224, 224], batch_size=8, 'dynamic')`` (one
64-frame ``_process_frame`` chunk, dama.py:179-186) under bf16 autocast,
``combined_loss`` at epoch=1/max_epochs=1 (BCE + orthogonal term), backward,
Adam(lr 1e-4, wd 1e-4) step.  Random-init weights, N(0,1) frames.  The iteration
is recorded once into HIP graphs and replayed (ewvit/graph.py; --eager issues
every launch from Python instead).

Multi-GPU: one process per GPU.  `python bench.py --gpus N` (no torchrun env) starts N
ranks itself through torch.distributed.run before touching the GPU and relays rank 0's
line; under torchrun it checks WORLD_SIZE == N.  Each replayed step broadcasts rank 0's
BN buffers, runs forward + backward with the gradient all-reduces (RCCL over xGMI,
bucketed, issued as buckets fill so they overlap the rest of the backward) and the
optimizer — all in one HIP graph (ewvit/graph.py); every rank runs its own 64-frame chunk
(weak scaling; BatchNorm statistics per rank like the reference's per-replica
DataParallel semantics).  value = all frames / max-over-ranks time.
EWVIT_BENCH_REHEARSE=1 puts every rank on cuda:0 over gloo (eager; timings meaningless):
the one-GPU rehearsal of the N-rank path.

A plain run sets up, warms up, times the K steps and prints the result line (metric, value,
unit, higher_is_better, dtype, ms_per_step, the workload's config).  --full adds everything
that takes runs of its own: the per-kernel event passes with their rooflines, the isolated DWT
front-end timing and the CPU baseline (--no-cpu-baseline drops the last).  --dump-outputs DIR
writes what the last timed step produced (dump_outputs: loss, parameters) as DIR/<name>.npy.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full [--no-cpu-baseline]]
                       [--dump-outputs DIR] [--eager]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, 'efficient-wavelet-vit_amd'))

METRIC = 'frames/sec fwd+bwd, 224×224 bs=64 dim=128, at 1/2/4/8 MI355X'
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
BF16_PEAK_TFS = 2500.0     # dense bf16 MFMA (spec, no sparsity)
FP8_PEAK_TFS = 5000.0      # dense fp8 e4m3 MFMA (spec, no sparsity)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', type=int, default=2, choices=(2, 3, 4, 5),
                    help='BASELINE.json configs[k-1]: 2 = 224^2 64 frames dim 128 (3 = the same per GPU on '
                         'N GPUs), 4 = MWT branch at 384^2 32 frames dim 256, 5 = fp8 token GEMMs, 128 frames')
    ap.add_argument('--frames', type=int, default=None, help='frames per GPU per step (config default)')
    ap.add_argument('--full', action='store_true',
                    help='also run the per-kernel event passes (rooflines, kernel table, isolated DWT timing) '
                         'and the CPU baseline; a plain run only times the steps')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--cpu-steps', type=int, default=4)
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps write the last step\'s loss and the parameters it left as '
                         'DIR/<name>.npy (float32)')
    ap.add_argument('--eager', action='store_true', help='issue every launch from Python (no HIP graph)')
    return ap.parse_args()


CONFIGS = {
    # BASELINE.json configs[1] / [2]: one 64-frame _process_frame chunk (8 videos x 8 frames)
    2: dict(image=224, dim=128, frames=64, videos=8, chunk=8, gemm='bf16'),
    3: dict(image=224, dim=128, frames=64, videos=8, chunk=8, gemm='bf16'),
    # configs[4]: 128 frames = 16 videos x 8 frames in 2 chunks of 64 (batch_size=4: a
    # 128-frame chunk overflows pos_embedding[0:N] in the reference, sfe.py:126,158-159)
    5: dict(image=224, dim=128, frames=128, videos=16, chunk=4, gemm='fp8'),
}


def _gemm(config):
    """The token GEMMs' precision of a config; EWVIT_BENCH_GEMM=bf16|fp8 overrides it for A/Bs
    (the line's dtype and config.token_gemms report what ran)."""
    g = os.environ.get('EWVIT_BENCH_GEMM') or CONFIGS.get(config, {}).get('gemm', 'bf16')
    if g not in ('bf16', 'fp8'):
        raise SystemExit(f'bench.py: EWVIT_BENCH_GEMM={g!r} (bf16 | fp8)')
    return g


def build_mwt_step(dev, frames, rank, graph=True):
    """BASELINE.json configs[3]: the MWT branch (mwt.py:92-119) at 384^2, 32 frames, dim 256,
    3 DWT levels — the reference's SFE cannot run at 384^2 (its 12x12 backbone map is not
    divisible by the 7x7 patch, sfe.py:153), so the step is MWT forward + a mean-square loss
    on its [N, 256, 1, 1] features + backward + Adam, bf16 autocast."""
    from network.mwt import MWT
    import ewvit
    from ewvit.graph import TrainStep
    torch.manual_seed(0)
    model = MWT(3, 256, 3).to(dev).to(memory_format=torch.channels_last).train()
    opt = ewvit.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4)
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    x = torch.randn(frames, 3, 384, 384, device=dev, generator=g)

    def forward_loss():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y = model(x)
        return y.float().square().mean()
    return TrainStep(model, forward_loss, opt, graph=graph)


def build_step(dev, frames, rank, graph=True, config=2, force_collectives=False):
    """The config's TrainStep (force_collectives: the test switch that issues the bucket
    all-reduces and the buffer broadcast in a world of one, ewvit/graph.py)."""
    if config == 4:
        return build_mwt_step(dev, frames, rank, graph)
    from network.model import DeepfakeDetector
    from network.losses import combined_loss, orth_weight
    import ewvit
    from ewvit.graph import TrainStep
    torch.manual_seed(0)                                   # identical init on every rank
    cfg = CONFIGS[config]
    videos = cfg['videos'] * frames // cfg['frames']
    gemm = _gemm(config)
    per_video = frames // videos
    chunk = cfg['chunk']                                   # frames per video per _process_frame call
    model = DeepfakeDetector(3, 128, batch_size=chunk).to(dev).to(memory_format=torch.channels_last)
    if gemm != 'bf16':
        from network import set_gemm_precision
        set_gemm_precision(model, gemm)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = ewvit.optim.Adam(params, lr=1e-4, weight_decay=1e-4)      # train.py:273-275 on csrc/optim.hip
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([0.5], device=dev))
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    x = torch.randn(videos, per_video, 3, 224, 224, device=dev, generator=g)
    gl = torch.Generator(device=dev).manual_seed(2000 + rank)
    y = torch.bernoulli(torch.full((videos,), 0.5, device=dev), generator=gl)
    model.train()

    # the curriculum weight of the orthogonality term as a device scalar (epoch 1 of 1: 1.0),
    # so a replayed step would follow an epoch schedule written in place
    orth_w = torch.full((), orth_weight(1, 1), device=dev)

    def forward_loss():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = model(x, chunk, 'dynamic')
        loss, _ = combined_loss(out, y, crit, 1, 1, weight=orth_w)
        return loss
    # gradients averaged over ranks by bucketed RCCL all-reduces issued during backward;
    # the whole iteration replayed from one HIP graph (ewvit/graph.py).  EWVIT_EARLY_STEP=1 (A/B,
    # measured slower): everything but the backbone takes its Adam update as soon as its
    # gradients are final, beside the backbone's backward (TrainStep early_params)
    backbone = {id(p) for p in model.dama.sfe.efficient_net.parameters()}
    early = [p for p in params if id(p) not in backbone]
    return TrainStep(model, forward_loss, opt, graph=graph, force_collectives=force_collectives, early_params=early)


def kernel_table(records):
    """Per ewvit entry point: launches, mean duration, algorithmic rate."""
    table = {}
    for name, recs in records.items():
        if name.startswith('__'):
            continue
        ms = [s.elapsed_time(e) for s, e, _ in recs]
        if not ms:
            continue
        tot = sum(ms)
        byt = sum(w.get('bytes', 0.0) for _, _, w in recs)
        fl = sum(w.get('flops', 0.0) for _, _, w in recs)
        table[name] = {'launches': len(ms), 'total_ms': tot, 'avg_us': 1e3 * tot / len(ms),
                       'GB/s': byt / (tot * 1e-3) / 1e9 if tot else 0.0,
                       'TFLOP/s': fl / (tot * 1e-3) / 1e12 if tot else 0.0,
                       'bytes_per_launch': byt / len(ms), 'flops_per_launch': fl / len(ms)}
    return table


def shape_table(detail):
    """Per (entry point, integer arguments = one launch configuration): launches,
    total, mean duration and algorithmic rate — the hottest single kernel configuration."""
    rows = {}
    for name, ints, s, e, w in detail:
        r = rows.setdefault((name, ints), {'ms': [], 'bytes': 0.0, 'flops': 0.0})
        r['ms'].append(s.elapsed_time(e))
        r['bytes'] += w.get('bytes', 0.0)
        r['flops'] += w.get('flops', 0.0)
    out = []
    for (name, ints), r in rows.items():
        tot = sum(r['ms'])
        out.append({'entry': name, 'args': list(ints), 'launches': len(r['ms']), 'total_ms': tot,
                    'avg_us': 1e3 * tot / len(r['ms']),
                    'GB/s': r['bytes'] / (tot * 1e-3) / 1e9 if tot else 0.0,
                    'TFLOP/s': r['flops'] / (tot * 1e-3) / 1e12 if tot else 0.0,
                    'bytes_per_launch': r['bytes'] / len(r['ms']), 'flops_per_launch': r['flops'] / len(r['ms'])})
    return sorted(out, key=lambda r: -r['total_ms'])


# device kernels behind each C-ABI entry point (for the PMC traffic lookup)
ENTRY_KERNELS = {
    'ewvit_dwt_haar_fwd': ['dwt_multilevel_kernel'],
    'ewvit_hf_upsample': ['hf_upsample_kernel'],
    'ewvit_dwt_hf_upsample_fused': ['dwt_hf_fused_kernel'],
    'ewvit_gemm': ['gemm_kernel', 'splitk_reduce_kernel'],
    'ewvit_gemm_mx8': ['gemm_mx8_kernel'],
    'ewvit_dwconv3x3_fwd': ['dw_row_bf16_kernel<1, false>', 'dw_row_bf16_kernel<2, false>', 'dw_fwd_kernel'],
    'ewvit_dwconv3x3_bwd_data': ['dw_row_bf16_kernel<1, true>', 'dw_bwd_data_kernel'],
    'ewvit_dwconv3x3_bwd_weight': ['dw_wgrad_row_bf16_kernel', 'dw_bwd_weight_partial_kernel',
                                   'dw_bwd_weight_reduce_kernel'],
    'ewvit_dwconv3x3_bwd_fused': ['dw_row4_kernel<2, 0, true>', 'dw_row4_kernel<2, 1, true>',
                                  'dw_row4_kernel<2, 2, true>'],
    'ewvit_conv2d_fwd': ['conv_fwd_kernel<false', 'conv_glds_kernel<false', 'conv_win_kernel<false, false, false'],
    'ewvit_conv2d_bwd_data': ['conv_fwd_kernel<true', 'conv_glds_kernel<true', 'conv_win_kernel<true, false, false, false'],
    'ewvit_conv2d_bwd_weight': ['conv_wgrad_kernel', 'conv_wgrad_glds_kernel', 'conv_wgrad_1x1_kernel',
                                'conv_wgrad_win_kernel<true, false', 'conv_wgrad_win_kernel<false, false',
                                'conv_wgrad_reduce_kernel', 'red_jobs_kernel'],
    # the windowed MWT convs (csrc/convwin.hip): the input-gradient kernels with the BatchNorm
    # backward sums in their epilogue, the forward / weight gradient with the folded input
    # transform (XF); template arguments <DGRAD, STATS, XF, BST, KS> / <BIAS, XF, TS>.  The
    # weight-gradient slabs' reduce pass is counted under ewvit_conv2d_bwd_weight only
    'ewvit_conv2d_bwd_data_bn_win': ['conv_win_kernel<true, false, false, true'],
    'ewvit_conv2d_fwd_bn': ['conv_win_kernel<false, true, false'],
    'ewvit_conv2d_fwd_bn_xf': ['conv_win_kernel<false, true, true'],
    'ewvit_conv2d_bwd_weight_xf': ['conv_wgrad_win_kernel<true, true', 'conv_wgrad_win_kernel<false, true'],
    'ewvit_bn_fwd': ['bn_stats_kernel', 'bn_apply_kernel'],
    'ewvit_bn_bwd': ['bn_bwd_reduce_kernel', 'bn_bwd_dx_kernel'],
    'ewvit_se_reduce': ['se_reduce_kernel', 'se_fold_kernel'],
    'ewvit_se_scale': ['se_scale_kernel'],
    'ewvit_scale_add': ['scale_add_kernel'],
}
MFMA_ENTRIES = ('ewvit_gemm', 'ewvit_gemm_mx8', 'ewvit_gemm_tallk', 'ewvit_conv2d_fwd', 'ewvit_conv2d_bwd_data',
                'ewvit_conv2d_bwd_weight')
NON_MFMA_CONV = ('ewvit_conv2d_pack_weights', 'ewvit_conv2d_stem_fwd')   # VALU / copy entry points
# MXFP8 entry points (v_mfma_scale_f32_16x16x128_f8f6f4 runs at the fp8 rate, MI355X_MICROARCH.md)
FP8_ENTRIES = ('ewvit_gemm_mx8',)


def is_mfma(name):
    """Entry points whose work is MFMA GEMM: the GEMMs and every implicit-GEMM conv variant
    (_bn / _xf / _win / _add forms of fwd, bwd_data, bwd_weight)."""
    return name in MFMA_ENTRIES or (name.startswith('ewvit_conv2d_') and name not in NON_MFMA_CONV)
def pmc_file(config):
    return os.path.join(REPO, 'profiles', 'pmc_latest.json' if config in (2, 3) else f'pmc_latest_c{config}.json')


# entry points that launch exactly one kernel per call: traffic per call = bytes per dispatch
PER_DISPATCH = ('ewvit_dwt_haar_fwd', 'ewvit_hf_upsample', 'ewvit_dwt_hf_upsample_fused')


def pmc_traffic(entry, per_step, config=2, adam_per_step=None):
    """HBM bytes per launch of `entry` from the committed rocprofv3 PMC passes of the same
    bench config (tools/gpu_pmc.sh: FETCH_SIZE x2 + WRITE_SIZE), or None.  The profiled bench
    run also executes the eager timing passes and the DWT loop, so the number of step
    equivalents it ran is counted from the Adam launches it made (Adam runs once per step in
    every pass; `adam_per_step` maps each Adam kernel name to its launches per step, so a
    PMC file from either launch form counts right), not from the command line."""
    path = pmc_file(config)
    if not os.path.exists(path) or entry not in ENTRY_KERNELS:
        return None
    data = json.load(open(path))
    if data.get('_config', 2) not in ((2, 3) if config in (2, 3) else (config,)):
        return None
    ks = [v for k, v in data.items() if not k.startswith('_') and any(p in k for p in ENTRY_KERNELS[entry])]
    if not ks:
        return None
    tot = sum(v['hbm_bytes_per_launch'] * v['dispatches'] for v in ks)
    if entry in PER_DISPATCH:
        return round(tot / sum(v['dispatches'] for v in ks), 1)
    # {kernel name: launches per step}; a run may mix the forms (eager passes vs a graph
    # captured with the other), so the step equivalents of each form add up
    counted = [sum(v['dispatches'] for k, v in data.items() if kname in k) / per
               for kname, per in (adam_per_step or {}).items() if per]
    steps = sum(counted) if any(counted) else data.get('_steps_executed')
    if not steps or not per_step:
        return None
    return round(tot / (per_step * steps), 1)


def _mwt_cap():
    from network import dama
    return dama._mwt_grid_cap()


def roofline_for(name, row, config=2, adam_per_step=None):
    traffic = pmc_traffic(name, row.get('per_step'), config, adam_per_step)
    if is_mfma(name):
        ach = row['TFLOP/s']
        peak = FP8_PEAK_TFS if name in FP8_ENTRIES else BF16_PEAK_TFS
        # traffic / the bytes the kernels must move (every tensor they read or write once,
        # including the BatchNorm inputs their epilogues and operand transforms read)
        ratio = round(traffic / row['bytes_per_launch'], 4) if traffic and row.get('bytes_per_launch') else None
        return {'kernel': name, 'bound': 'mfma', 'achieved': round(ach, 3), 'peak': peak,
                'unit': 'TFLOP/s', 'frac': round(ach / peak, 5), 'traffic': traffic,
                'avg_us': round(row['avg_us'], 3), 'work_per_launch': row['flops_per_launch'],
                'algorithmic_bytes_per_launch': row['bytes_per_launch'], 'traffic_ratio': ratio}
    ach = row['GB/s']
    return {'kernel': name, 'bound': 'hbm', 'achieved': round(ach, 2), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
            'frac': round(ach / HBM_PEAK_GBS, 5), 'traffic': traffic, 'avg_us': round(row['avg_us'], 3),
            'work_per_launch': row['bytes_per_launch']}


def mfma_util(table, ms_per_step):
    """Step-level MFMA utilisation: the algorithmic GEMM / conv flops of one step (every MFMA
    entry point's launches of the eager pass, per step) over the timed step, against the dense
    bf16 peak (config 2: ~4.32 TFLOP per 64-frame step)."""
    fl = sum(r['flops_per_launch'] * r['per_step'] for n, r in table.items() if is_mfma(n))
    ach = fl / (ms_per_step * 1e-3) / 1e12
    return {'flops_per_step': fl, 'achieved': round(ach, 2), 'peak': BF16_PEAK_TFS, 'unit': 'TFLOP/s',
            'frac': round(ach / BF16_PEAK_TFS, 5)}


def cpu_baseline(steps, config=2):
    """The oracle (CPU fp32 eager restatement of the reference, same op sequence)
    timed on this host: 8-frame chunk, fwd+bwd+Adam; config 4: the MWT
    branch at 384^2 dim 256 on 2-frame steps."""
    sys.path.insert(0, REPO)
    from oracle import model as om
    threads = len(os.sched_getaffinity(0))
    threads = min(threads, int(os.environ.get('OMP_NUM_THREADS', threads)))
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    if config == 4:
        m = om.MWT(3, 256, 3).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-4)
        x = torch.randn(2, 3, 384, 384)

        def mstep():
            m(x).square().mean().backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        mstep()
        n = max(1, steps // 2)
        t = time.perf_counter()
        for _ in range(n):
            mstep()
        dt = time.perf_counter() - t
        return {'value': round(2 * n / dt, 4), 'unit': 'frames/s', 'cores': threads, 'kind': 'port',
                'sample': f'oracle fp32 eager MWT(3,256,3) at 384^2, {n} steps x 2 frames fwd+bwd+Adam, after 1 warm-up'}
    m = om.DeepfakeDetector(3, 128, batch_size=8)
    m.train()
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4)
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([0.5]))
    x = torch.randn(1, 8, 3, 224, 224)
    y = torch.tensor([1.0])

    def step():
        out = m(x, 8, 'dynamic')
        om.combined_loss(out, y, crit, 1, 1).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    step()
    t = time.perf_counter()
    for _ in range(steps):
        step()
    dt = time.perf_counter() - t
    return {'value': round(8 * steps / dt, 3), 'unit': 'frames/s', 'cores': threads, 'kind': 'port',
            'sample': f'oracle fp32 eager, {steps} steps x 8 frames (1 chunk) fwd+bwd+Adam, after 1 warm-up'}


def workload(args, world, step):
    if args.config == 4:
        return {'workload': 'BASELINE configs[3]: MWT branch train step (mwt.py:92-119) fwd + mean-square loss + '
                            'bwd + Adam at 384x384, 3 DWT levels', 'image': 384, 'frames_per_gpu': args.frames,
                'dim': 256, 'levels': 3, 'global_batch': args.frames * world, 'parallelism': f'dp{world}',
                'launch': step.mode, 'baseline_config': 4}
    cfg = CONFIGS[args.config]
    return {'workload': 'DAMA train step: DeepfakeDetector dynamic fwd + combined_loss + bwd + Adam',
            'image': 224, 'frames_per_gpu': args.frames, 'dim': 128, 'chunk_frames': cfg['videos'] * cfg['chunk'],
            'token_gemms': _gemm(args.config), 'global_batch': args.frames * world, 'parallelism': f'dp{world}',
            'launch': step.mode, 'baseline_config': 3 if world > 1 else args.config}


DUMP_MAX_ELEMS = 7_000_000     # 28 MB of float32: the dump stays well under 64 MB


def dump_outputs(step, out_dir):
    """What the last timed step left its caller, as DIR/<name>.npy (float32): `loss`, the value
    step() returned, and `params`, the trainable parameters after that step's Adam update,
    flattened in model.parameters() order and concatenated.  A concatenation longer than
    DUMP_MAX_ELEMS is cut to a fixed sample: the sorted first DUMP_MAX_ELEMS indices of a
    permutation seeded with 0, the same for every run.  Inputs, initial weights and dropout
    seeds are the same from run to run; the step's results are not bit-identical between runs
    ("Known: results differ from run to run": after 25 steps the parameters differ by
    about 1.2e-3 relative L2)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    params = [p for p in step.model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    flat = torch.cat([p.detach().float().flatten() for p in params])
    if n > DUMP_MAX_ELEMS:
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
        flat = flat[perm[:DUMP_MAX_ELEMS].sort().values.to(flat.device)]
    np.save(os.path.join(out_dir, 'loss.npy'), step.loss.detach().float().reshape(-1).cpu().numpy())
    np.save(os.path.join(out_dir, 'params.npy'), flat.cpu().numpy())


def kernel_passes(step, args):
    """--full: the per-kernel event passes after the timed loop -> (table, shapes, iso_table, kt)."""
    import ewvit
    # per-kernel timing pass (HIP events around every ewvit launch, separate from the timed
    # loop): the same iteration issued eagerly, so each launch can be bracketed
    ewvit._lib.enable_timing(True)
    kt = max(3, min(args.steps, 5))
    for _ in range(kt):
        step._eager()
    torch.cuda.synchronize()
    table = kernel_table(ewvit._lib.timing_records())
    shapes = shape_table(ewvit._lib.timing_detail())
    ewvit._lib.enable_timing(False)
    for r in table.values():
        r['per_step'] = r['launches'] / kt
    # the same pass with the MWT on the main stream and uncapped grids: each kernel on the
    # whole chip (the timed step runs the MWT's big launches on 128 of the 256 CUs, beside
    # the backbone — network/dama.py _mwt_grid_cap — so their as-run durations are longer)
    # (every rank runs it: the eager step issues the gradient all-reduces and the buffer
    # broadcast, so a rank-0-only pass would wait on its peers forever)
    iso_table = None
    if args.config in (2, 3, 5):
        saved = {k: os.environ.get(k) for k in ('EWVIT_BRANCH_STREAMS', 'EWVIT_MWT_GRID_CAP')}
        os.environ['EWVIT_BRANCH_STREAMS'] = '0'
        os.environ['EWVIT_MWT_GRID_CAP'] = '0'
        try:
            ewvit._lib.enable_timing(True)
            for _ in range(kt):
                step._eager()
            torch.cuda.synchronize()
            iso_table = kernel_table(ewvit._lib.timing_records())
            ewvit._lib.enable_timing(False)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        for r in iso_table.values():
            r['per_step'] = r['launches'] / kt
    return table, shapes, iso_table, kt


def full_report(res, step, args, table, shapes, iso_table, kt):
    """--full: the rooflines, the kernel table, the isolated DWT timing and the CPU baseline of the line."""
    dom = max(table.items(), key=lambda kv: kv[1]['total_ms']) if table else None
    if table:
        res['mfma_util'] = mfma_util(table, res['ms_per_step'])
    opt = getattr(step, 'opt', None)
    aps = opt.launches_per_step() if hasattr(opt, 'launches_per_step') else None
    res['roofline'] = roofline_for(*dom, config=args.config, adam_per_step=aps) if dom else None
    if res['roofline'] is not None:
        cap = _mwt_cap()
        res['roofline']['timing'] = ('HIP events around every launch of an eager pass of the step as it runs '
                                     f'(MWT on its own stream, its big grids capped at {cap} workgroups)')
    if iso_table and dom and dom[0] in iso_table:
        iso = roofline_for(dom[0], iso_table[dom[0]], config=args.config, adam_per_step=aps)
        iso['timing'] = 'same pass with one stream and uncapped grids (each kernel on the whole chip)'
        res['roofline_isolated'] = iso
    if shapes:
        # the hottest single launch configuration (entry point + shape arguments)
        h = dict(shapes[0])
        h['per_step'] = h['launches'] / kt
        hot = roofline_for(h['entry'], h, args.config, aps)
        hot['traffic'] = None      # the PMC passes are summarised per kernel symbol, not per shape
        hot['args'] = h['args']
        res['roofline_hot'] = hot
        res['top_launch_configs'] = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
                                     for r in shapes[:12]]
    # MFMA utilisation of the token path's GEMMs (ViT attention / MLP projections,
    # patch_to_embedding, classifier: north_star's attention/MLP figure); at config 5 the
    # attention / MLP projections are the fp8 entry point, priced against the fp8 peak
    tok = 'ewvit_gemm_mx8' if (args.config == 5 and 'ewvit_gemm_mx8' in table) else 'ewvit_gemm'
    if tok in table:
        tg = roofline_for(tok, table[tok], args.config, aps)
        tg['timing'] = res['roofline']['timing'] if res.get('roofline') else None
        tg['launches_per_step'] = table[tok]['per_step']
        res['token_gemm_roofline'] = tg
    res['kernels'] = {k: {kk: (round(vv, 4) if isinstance(vv, float) else vv) for kk, vv in v.items()}
                      for k, v in sorted(table.items(), key=lambda kv: -kv[1]['total_ms'])}
    fe = next((e for e in ('ewvit_dwt_hf_upsample_fused', 'ewvit_dwt_haar_fwd') if e in table), None)
    if fe is not None:
        # the MWT front end: the fused DWT -> HF upsample launch (or the DWT of the two-launch
        # path).  The per-launch events of the eager pass add ~10 us around a ~20 us kernel:
        # the achieved rate is taken from back-to-back launches on the same frames replayed
        # from one HIP graph (tools/dwt_bench.py; matches rocprofv3's kernel duration)
        dr = roofline_for(fe, table[fe], args.config, aps)
        sys.path.insert(0, os.path.join(REPO, 'tools'))
        import dwt_bench
        iso = dwt_bench.measure(n=args.frames, hw=384 if args.config == 4 else 224, levels=3)
        k = 'fused' if fe == 'ewvit_dwt_hf_upsample_fused' else 'dwt'
        dr['event_avg_us'] = dr['avg_us']
        dr['avg_us'] = round(iso[k + '_us'], 3)
        dr['work_per_launch'] = iso[k + '_bytes']
        dr['achieved'] = round(iso[k + '_bytes'] / iso[k + '_us'] / 1e3, 2)
        dr['frac'] = round(dr['achieved'] / HBM_PEAK_GBS, 5)
        dr['timing'] = 'HIP graph of 50 back-to-back launches, events around the replay'
        dr['channels'] = iso['channels']      # hf_conv input channels written (9: the real bands)
        # the two-launch path it replaces, same frames: DWT (bands to HBM) + upsample
        dr['two_launch'] = {n: {'avg_us': round(iso[n + '_us'], 3), 'work_per_launch': iso[n + '_bytes'],
                                'achieved': round(iso[n + '_bytes'] / iso[n + '_us'] / 1e3, 2),
                                'frac': round(iso[n + '_bytes'] / iso[n + '_us'] / 1e3 / HBM_PEAK_GBS, 5)}
                            for n in ('dwt', 'up')}
        res['dwt_roofline'] = dr
    res['cpu_baseline'] = None if args.no_cpu_baseline else cpu_baseline(args.cpu_steps, args.config)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n):
    """--gpus N outside torchrun: start N ranks (one process per GPU) as a child
    torch.distributed.run — before this process touches the GPU — and exit with its code.
    Rank 0's JSON line reaches stdout through the inherited file descriptors."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}',
           '--master-addr=127.0.0.1', f'--master-port={_free_port()}', os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    import ewvit
    from ewvit import dist as edist
    edist.rccl_env()        # fresh collective events (no captured event reaches the watchdog), FR status
    rank, world, local = edist.env_ranks()
    if world != args.gpus:
        print(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a mislabelled '
              f'n_gpus', file=sys.stderr, flush=True)
        sys.exit(2)
    # EWVIT_BENCH_REHEARSE=1: every rank on cuda:0 over gloo — exercises the DDP path
    # on a one-GPU box (timings meaningless); the real run is one rank per GPU on RCCL
    rehearse = os.environ.get('EWVIT_BENCH_REHEARSE') == '1'
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    edist.init_from_env('gloo' if rehearse else 'nccl')    # RCCL over xGMI
    ewvit.load_library()                       # fail loudly if the HIP library is missing
    if args.frames is None:
        args.frames = 32 if args.config == 4 else CONFIGS[args.config]['frames']
    step = build_step(dev, args.frames, rank, graph=not args.eager, config=args.config)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    edist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    edist.barrier()
    torch.cuda.synchronize()
    elapsed = edist.max_over_ranks(time.perf_counter() - t0, dev)

    if args.dump_outputs and rank == 0:
        dump_outputs(step, args.dump_outputs)        # before --full's event passes run further steps
    if args.full:
        table, shapes, iso_table, kt = kernel_passes(step, args)

    if rank == 0:
        frames = args.frames * world * args.steps
        metric = METRIC if args.config in (2, 3) else {
            4: 'frames/sec fwd+bwd, 384×384 bs=32 dim=256 3-level DWT, MWT branch, MI355X',
            5: 'frames/sec fwd+bwd, 224×224 bs=128 dim=128, fp8 e4m3 token GEMMs, MI355X'}[args.config]
        res = {'metric': metric, 'value': round(frames / elapsed, 2), 'unit': 'frames/s', 'n_gpus': world,
               'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(1e3 * elapsed / args.steps, 3),
               'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
               # config 5: the attention / MLP token GEMMs on fp8 e4m3 operands, everything else bf16
               'dtype': 'fp8e4m3+bf16' if _gemm(args.config) == 'fp8' else 'bf16',
               'data': 'synthetic N(0,1) frames, random-init weights (no datasets/checkpoints offline)',
               'config': workload(args, world, step)}
        res['allreduce'] = step.describe() if hasattr(step, 'describe') else None
        if args.full:
            full_report(res, step, args, table, shapes, iso_table, kt)
        print(json.dumps(res), flush=True)
    if hasattr(step, 'close'):
        step.close()                 # graphs holding RCCL collectives released before the communicator
    if world > 1 and dist.is_initialized():
        edist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

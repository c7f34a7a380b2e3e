"""bench.py's roofline reporting (host logic only, no GPU): each MFMA entry point is priced
against the dense peak of the dtype it computes in, HBM-bound entries against HBM3E."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _row(tfs, gbs):
    return {'TFLOP/s': tfs, 'GB/s': gbs, 'avg_us': 10.0, 'flops_per_launch': 1e9, 'bytes_per_launch': 1e6,
            'per_step': 1.0}


def test_fp8_gemm_priced_against_fp8_peak():
    import bench
    r = bench.roofline_for('ewvit_gemm_mx8', _row(500.0, 0.0), config=5)
    assert r['bound'] == 'mfma' and r['peak'] == bench.FP8_PEAK_TFS == 5000.0
    assert abs(r['frac'] - 0.1) < 1e-9


def test_bf16_gemm_and_conv_priced_against_bf16_peak():
    import bench
    for name in ('ewvit_gemm', 'ewvit_conv2d_bwd_weight'):
        r = bench.roofline_for(name, _row(250.0, 0.0))
        assert r['peak'] == bench.BF16_PEAK_TFS and abs(r['frac'] - 0.1) < 1e-9


def test_hbm_entry_priced_against_hbm():
    import bench
    r = bench.roofline_for('ewvit_bn_bwd', _row(0.0, 4000.0))
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and abs(r['frac'] - 0.5) < 1e-9


def test_conv_variants_priced_as_mfma():
    """the windowed / BatchNorm-fused conv entry points are MFMA work; pack / stem are not"""
    import bench
    for name in ('ewvit_conv2d_bwd_data_bn_win', 'ewvit_conv2d_fwd_bn_xf', 'ewvit_conv2d_bwd_weight_xf',
                 'ewvit_conv2d_fwd_bn', 'ewvit_conv2d_bwd_data_add', 'ewvit_gemm_tallk'):
        assert bench.roofline_for(name, _row(250.0, 0.0))['bound'] == 'mfma', name
    for name in ('ewvit_conv2d_pack_weights', 'ewvit_conv2d_stem_fwd'):
        assert bench.roofline_for(name, _row(0.0, 800.0))['bound'] == 'hbm', name


def test_pmc_patterns_cover_windowed_kernels():
    """every windowed conv kernel symbol maps to exactly one entry point (no double counting)"""
    import bench
    syms = ['void ewvit::conv_win_kernel<true, false, false, true, false>(ewvit::FwdArgs, long, long, int, int, int)',
            'void ewvit::conv_win_kernel<true, false, false, true, true>(ewvit::FwdArgs, long, long, int, int, int)',
            'void ewvit::conv_win_kernel<false, true, true, false, false>(ewvit::FwdArgs, long, long, int, int, int)',
            'void ewvit::conv_wgrad_win_kernel<true, true, true>(ewvit::WgradArgs, long, int, int, int, int)',
            'void ewvit::conv_wgrad_win_kernel<true, false, true>(ewvit::WgradArgs, long, int, int, int, int)',
            'void ewvit::conv_wgrad_1x1_kernel<2>(ewvit::WgradArgs, int, int)',
            'void ewvit::conv_win_kernel<false, true, false, false, false>(ewvit::FwdArgs, long, long, int, int, int)',
            'void ewvit::conv_win_kernel<true, false, false, false, false>(ewvit::FwdArgs, long, long, int, int, int)',
            'void ewvit::conv_win_kernel<false, false, false, false, false>(ewvit::FwdArgs, long, long, int, int, int)',
            'void ewvit::conv_glds_kernel<true, 128, 64, 3, 2, 4, false, true>(ewvit::FwdArgs, long, int, int, int)']
    for k in syms:
        owners = [e for e, pats in bench.ENTRY_KERNELS.items() if any(p in k for p in pats)]
        assert len(owners) == 1, (k, owners)


def test_dominant_dgrad_traffic_ratio_matches_hand_count():
    """The line's traffic / algorithmic-bytes ratio for the windowed input gradient with the
    BatchNorm-backward sums (ewvit_conv2d_bwd_data_bn_win, 2 launches per config-2 step),
    recomputed by hand from the shapes: the multiscale dgrad reads dy [64, 112^2, 128] and the
    BN input z [3 x 64, 112^2, 128], writes dx [3 x 64, 112^2, 128]; the k-split fusion dgrad
    reads dy [192, 112^2, 128] and the seperate BN's input [192, 112^2, 64], writes dx [192,
    112^2, 64] (bf16; the packed weights < 1 MB).  Against the committed PMC pass the ratio is
    ~1.06 (multiscale 1.11, fusion 1.01): the windows' halos, not a missing tensor."""
    import json
    import bench
    px = 64 * 112 * 112
    ms = (px * 128 + 3 * px * 128 + 3 * px * 128) * 2 + 128 * 384 * 9 * 2
    fu = (3 * px * 128 + 3 * px * 64 + 3 * px * 64) * 2 + 64 * 128 * 9 * 2
    hand = (ms + fu) / 2
    data = json.load(open(bench.pmc_file(2)))
    adam = {k: v for k, v in data.items() if 'adam_table_kernel' in k}
    row = dict(_row(300.0, 0.0), per_step=2.0, bytes_per_launch=hand)
    r = bench.roofline_for('ewvit_conv2d_bwd_data_bn_win', row, config=2,
                           adam_per_step={'adam_table_kernel': 1} if adam else None)
    assert r['traffic'] is not None
    assert r['traffic_ratio'] == round(r['traffic'] / hand, 4)
    assert 0.95 <= r['traffic_ratio'] <= 1.2, r['traffic_ratio']


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--no-cpu-baseline', '--dump-outputs', 'd'])
    a = bench.parse()
    assert a.full and a.no_cpu_baseline and a.dump_outputs == 'd'


def _run_main(monkeypatch, capsys, argv):
    """bench.main() on the host with a stub step in place of the GPU one: -> (the result line,
    the stub's call count, the --full functions that ran)."""
    import json
    import types
    import torch
    import bench
    import ewvit
    from ewvit import dist as edist
    model = torch.nn.Linear(3, 2)
    calls, ran = [], []

    class Step:
        mode, loss = 'graph', torch.tensor(0.25)

        def __init__(self):
            self.model = model

        def __call__(self):
            calls.append(1)
            return self.loss

        def _eager(self):
            raise AssertionError('a plain run issued an eager pass')

        def describe(self):
            return {'launch': 'hip-graph', 'world': 1}

        def close(self):
            pass
    for name in ('set_device', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, lambda *a, **k: None)
    monkeypatch.setattr(edist, 'rccl_env', lambda: None)
    monkeypatch.setattr(edist, 'env_ranks', lambda: (0, 1, 0))
    monkeypatch.setattr(edist, 'init_from_env', lambda *a, **k: None)
    monkeypatch.setattr(edist, 'barrier', lambda: None)
    monkeypatch.setattr(edist, 'max_over_ranks', lambda t, dev: t)
    monkeypatch.setattr(ewvit, 'load_library', lambda: None)
    monkeypatch.setattr(bench, 'build_step', lambda *a, **k: Step())

    def passes(step, args):
        ran.append('kernel_passes')
        return {}, [], None, 3

    def report(res, *a):
        ran.append('full_report')
        res['kernels'], res['roofline'], res['cpu_baseline'] = {}, None, None
    monkeypatch.setattr(bench, 'kernel_passes', passes)
    monkeypatch.setattr(bench, 'full_report', report)
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    bench.main()
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1                                # one JSON result line
    return json.loads(line[0]), len(calls), ran


def test_plain_run_times_the_steps_and_nothing_else(monkeypatch, capsys, tmp_path):
    """A plain run calls the step warmup + steps times, runs neither the event passes nor the
    report behind --full, and its line holds the headline fields without the --full ones."""
    res, n, ran = _run_main(monkeypatch, capsys, ['--gpus', '1', '--steps', '7', '--warmup', '2',
                                                  '--dump-outputs', str(tmp_path / 'd')])
    assert n == 9 and ran == []
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in res, k
    assert res['steps'] == 7 and res['warmup'] == 2 and res['unit'] == 'frames/s' and res['higher_is_better'] is True
    assert isinstance(res['ms_per_step'], float) and res['ms_per_step'] >= 0 and res['value'] > 0
    for k in ('kernels', 'roofline', 'roofline_isolated', 'roofline_hot', 'top_launch_configs', 'mfma_util',
              'token_gemm_roofline', 'dwt_roofline', 'cpu_baseline'):
        assert k not in res, k
    assert sorted(f.name for f in (tmp_path / 'd').iterdir()) == ['loss.npy', 'params.npy']


def test_full_run_adds_the_passes_and_the_report(monkeypatch, capsys):
    res, n, ran = _run_main(monkeypatch, capsys, ['--gpus', '1', '--steps', '3', '--warmup', '1', '--full'])
    assert n == 4 and ran == ['kernel_passes', 'full_report']
    assert 'kernels' in res and 'cpu_baseline' in res and 'ms_per_step' in res


def test_dump_outputs_writes_loss_and_params(tmp_path, monkeypatch):
    """float32 .npy files, the trainable parameters in model.parameters() order; a long
    concatenation is cut to the same seeded sample of indices, identical from call to call."""
    import types
    import numpy as np
    import torch
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3)).double()
    model[1].bias.requires_grad_(False)
    loss = model(torch.randn(4, 5).double()).square().mean().detach()
    step = types.SimpleNamespace(model=model, loss=loss)
    flat = torch.cat([p.detach().float().flatten() for p in model.parameters() if p.requires_grad]).numpy()
    assert flat.size == 5 * 7 + 7 + 7 * 3

    bench.dump_outputs(step, str(tmp_path / 'a'))
    assert sorted(f.name for f in (tmp_path / 'a').iterdir()) == ['loss.npy', 'params.npy']
    got = {n: np.load(tmp_path / 'a' / f'{n}.npy') for n in ('loss', 'params')}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got['loss'].shape == (1,) and got['loss'][0] == np.float32(loss.item())
    assert np.array_equal(got['params'], flat)

    monkeypatch.setattr(bench, 'DUMP_MAX_ELEMS', 10)
    bench.dump_outputs(step, str(tmp_path / 'b'))
    bench.dump_outputs(step, str(tmp_path / 'c'))
    idx = torch.randperm(flat.size, generator=torch.Generator().manual_seed(0))[:10].sort().values.numpy()
    b, c = np.load(tmp_path / 'b' / 'params.npy'), np.load(tmp_path / 'c' / 'params.npy')
    assert b.shape == (10,) and np.array_equal(b, c) and np.array_equal(b, flat[idx])


def test_dump_budget_is_under_64_mb():
    import bench
    assert 4 * (bench.DUMP_MAX_ELEMS + 1) <= 64 * 10 ** 6


def test_mfma_util_counts_mfma_entries_only():
    import bench
    table = {'ewvit_conv2d_fwd': dict(_row(0, 0), flops_per_launch=1e12, per_step=2.0),
             'ewvit_bn_bwd': dict(_row(0, 0), flops_per_launch=5e12, per_step=1.0)}
    u = bench.mfma_util(table, 1.0)          # 2 TFLOP in 1 ms = 2000 TFLOP/s
    assert u['flops_per_step'] == 2e12 and abs(u['achieved'] - 2000.0) < 1e-6 and abs(u['frac'] - 0.8) < 1e-9

"""CPU-side checks of the C-ABI boundary: the library loads, exports every
symbol include/ewvit.h declares, reports its ABI version, and rejects bad
arguments with an error message — no GPU compute is issued here."""
import ctypes
import os
import re

import pytest

from conftest import PKG, REPO

HEADER = os.path.join(REPO, 'include', 'ewvit.h')
LIB = os.path.join(PKG, 'ewvit', 'libewvit.so')


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r'\b(ewvit_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f'{LIB} not built (run __graft_entry__.build())')
    return ctypes.CDLL(LIB)


def test_every_declared_symbol_is_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/ewvit.h but not exported'


def test_python_binding_covers_the_header():
    from ewvit import _lib
    syms = set(declared_symbols()) - {'ewvit_abi_version', 'ewvit_last_error'}
    bound = set(_lib.SIGNATURES) | set(_lib.QUERIES)
    assert syms == bound, syms ^ bound


def test_abi_version(lib):
    lib.ewvit_abi_version.restype = ctypes.c_int
    from ewvit import _lib
    assert lib.ewvit_abi_version() == _lib.ABI_VERSION


def test_argument_errors_are_reported_without_gpu():
    from ewvit import _lib
    lib = _lib.load()
    # null operands -> EINVAL (1000) and a message; no HIP call is reached
    rc = lib.ewvit_dwt_haar_fwd(None, None, None, 1, 1, 8, 8, 1, 0, 0, None)
    assert rc == 1000
    assert b'null' in lib.ewvit_last_error()
    rc = lib.ewvit_dwt_haar_fwd(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 1, 1, 8, 8, 9, 0, 0, None)
    assert rc == 1000 and b'levels' in lib.ewvit_last_error()
    with pytest.raises(RuntimeError, match='unit stride'):
        _lib.call('ewvit_gemm', ctypes.c_void_p(16), 1, 7, 7, ctypes.c_void_p(16), 1, 1, 4,
                  ctypes.c_void_p(16), 0, 4, 4, 4, 4, 1.0, 0.0, None, 0, None, 0.0, 0, None, None, 0, 0, 1, None,
                  None)
    with pytest.raises(RuntimeError, match='nq=9'):
        _lib.call('ewvit_attn_fwd', ctypes.c_void_p(16), 0, 0, ctypes.c_void_p(16), 0, 0, ctypes.c_void_p(16),
                  0, 0, ctypes.c_void_p(16), 0, 0, None, 1, 1, 9, 2, 64, 1.0, None)


# ---- host-side argument checks of the BatchNorm / depthwise / squeeze-excitation entry points
# (csrc/batchnorm.hip, depthwise.hip, se.hip): every rejected call below returns EINVAL (1000)
# from a check that runs before any HIP call, with the entry's name in the message.
P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced

# name -> a full argument list that passes every check (never called as is)
GOOD = {
    # x y dtype M C gamma beta rmean rvar training momentum eps act smean sinvstd groups counter workspace stream
    'bn_fwd': [P, P, 1, 64, 16, P, P, P, P, 1, 0.1, 1e-3, 0, P, P, 1, P, P, None],
    # part_in nin shift_in part_out nout shift_out C groups stream
    'bn_fold_partials': [P, 4, P, P, 2, P, 16, 1, None],
    # x y dtype M C gamma beta rmean rvar momentum eps act smean sinvstd counter part shifts nrc groups stream
    'bn_fwd_partials': [P, P, 1, 64, 16, P, P, P, P, 0.1, 1e-3, 0, P, P, P, P, P, 4, 1, None],
    # M C gamma beta rmean rvar momentum eps smean sinvstd counter part shifts nrc groups coef stream
    'bn_coef': [64, 16, P, P, P, P, 0.1, 1e-3, P, P, P, P, P, 4, 1, P, None],
    # x y dtype M C gamma beta rmean rvar momentum eps smean sinvstd counter part shifts nrc skip HW keep seed
    # seed_offset scale_out workspace stream
    'bn_fwd_drop_add': [P, P, 1, 64, 16, P, P, P, P, 0.1, 1e-3, P, P, P, P, P, 4, P, 16, 0.9, 1, None, P, P, None],
    # dy x dx dtype M C gamma beta smean sinvstd dgamma dbeta row_scale HW workspace stream
    'bn_bwd_scaled': [P, P, P, 1, 64, 16, P, P, P, P, P, P, P, 16, P, None],
    # dy x dx dtype M C gamma beta smean sinvstd act dgamma dbeta se_s se_g HW workspace stream
    'bn_bwd_se': [P, P, P, 1, 64, 16, P, P, P, P, 0, P, P, P, P, 16, P, None],
    # dy x dx dtype M C gamma beta smean sinvstd act dgamma dbeta row_scale HW part nrc groups stream
    'bn_bwd_partials': [P, P, P, 1, 64, 16, P, P, P, P, 0, P, P, None, 0, P, 4, 1, None],
    # dy x dtype M C gamma beta smean sinvstd act groups part stream
    'bn_bwd_reduce': [P, P, 1, 64, 16, P, P, P, P, 0, 1, P, None],
    # dy x dx dtype M C gamma beta smean sinvstd act dgamma dbeta accumulate groups workspace stream
    'bn_bwd': [P, P, P, 1, 64, 16, P, P, P, P, 0, P, P, 0, 1, P, None],
    # x y dtype N HW C gamma beta rmean rvar momentum eps act smean sinvstd counter part shifts nrc w1 Csq s0
    # hpart stream
    'bn_act_se_squeeze': [P, P, 1, 2, 16, 16, P, P, P, P, 0.1, 1e-3, 2, P, P, P, P, P, 4, P, 4, P, P, None],
    # x w y N H W C stride pad dtype stream
    'dwconv3x3_fwd': [P, P, P, 2, 5, 5, 16, 1, 1, 1, None],
    'dwconv3x3_bwd_data': [P, P, P, 2, 5, 5, 16, 1, 1, 1, None],
    # x dy dw accumulate N H W C stride pad dtype workspace stream
    'dwconv3x3_bwd_weight': [P, P, P, 0, 2, 5, 5, 16, 1, 1, 1, P, None],
    # x w y N H W C stride shift part shift_out stream
    'dwconv3x3_fwd_bn': [P, P, P, 2, 5, 5, 16, 1, P, P, P, None],
    # dy w dx N H W C bx mean invstd gamma beta act part stream
    'dwconv3x3_bwd_data_bn': [P, P, P, 2, 5, 5, 16, P, P, P, P, P, 0, P, None],
    # dy w dx x dw accumulate N H W C bx mean invstd gamma beta act part workspace stream
    'dwconv3x3_bwd_fused': [P, P, P, P, P, 0, 2, 5, 5, 16, P, P, P, P, P, 0, P, P, None],
    # ... workspace z se_mean se_invstd se_gamma se_beta se_act se_row se_s se_g stream
    'dwconv3x3_bwd_fused_se': [P, P, P, P, P, 0, 2, 5, 5, 16, P, P, P, P, P, 0, P, P, P, P, P, P, P, 0, P, P, P, None],
    # a b dtype N HW C scale out workspace stream
    'se_reduce': [P, None, 1, 2, 9, 16, 1.0, P, P, None],
    # x dtype s g y N HW C stream
    'se_scale': [P, 1, P, None, P, 2, 9, 16, None],
    # r x dtype scale y N row_elems stream
    'scale_add': [P, None, 1, P, P, 2, 16, None],
    # r x dtype keep seed seed_offset scale_out y N row_elems stream
    'scale_add_drop': [P, P, 1, 0.9, 1, None, P, P, 2, 16, None],
    # s0 w1 b1 w2 b2 h1 s N C Csq workspace stream
    'se_mlp_fwd': [P, P, P, P, P, P, P, 2, 16, 4, P, None],
    # ds s h1 s0 w1 w2 inv_hw g dw1 db1 dw2 db2 N C Csq workspace stream
    'se_mlp_bwd': [P, P, P, P, P, P, 0.1, P, P, P, P, P, 2, 16, 4, P, None],
    # x dtype N HW C w1 b1 w2 b2 Csq s0 h1 s workspace stream
    'se_squeeze_mlp_fwd': [P, 1, 2, 9, 16, P, P, P, P, 4, P, P, P, P, None],
    # x dtype N HW C w1 b1 w2 b2 Csq s0 h1 s y workspace stream
    'se_forward': [P, 1, 2, 9, 16, P, P, P, P, 4, P, P, P, P, P, None],
    # part b1 w2 b2 x dtype N HW C Csq h1 s y stream
    'se_gate_excite': [P, P, P, P, P, 1, 2, 9, 16, 4, P, P, P, None],
    # dy x dtype N HW C s h1 s0 w1 w2 Csq g dw1 db1 dw2 db2 workspace stream
    'se_squeeze_mlp_bwd': [P, P, 1, 2, 9, 16, P, P, P, P, P, 4, P, P, P, P, P, P, None],
    # dy z dx dtype N HW C gamma beta smean sinvstd act s g row stream
    'bn_se_bwd_dx': [P, P, P, 1, 2, 9, 16, P, P, P, P, 0, P, P, P, None],
    # dy a z dx dtype N HW C gamma beta smean sinvstd act dgamma dbeta s h1 s0 w1 w2 Csq g dw1 db1 dw2 db2
    # workspace stream
    'bn_se_bwd': [P, P, P, P, 1, 2, 9, 16, P, P, P, P, 0, P, P, P, P, P, P, P, 4, P, P, P, P, P, P, None],
    # (csrc/pool.hip) x y argmax dtype N H W C stream
    'maxpool2_fwd': [P, P, P, 1, 1, 5, 5, 8, None],
    'maxpool2_bwd': [P, P, P, 1, 1, 5, 5, 8, None],
}

# (entry, {argument index: bad value}, a word the message must also hold or None)
REJECTED = [
    ('bn_fwd', {0: None}, None), ('bn_fwd', {2: 7}, None), ('bn_fwd', {4: 12}, None), ('bn_fwd', {12: 3}, None),
    ('bn_fwd', {15: 0}, None), ('bn_fwd', {15: 3}, None), ('bn_fwd', {9: 0, 7: None}, None),
    ('bn_fwd', {4: 4104}, None),
    ('bn_fold_partials', {0: None}, None), ('bn_fold_partials', {7: 0}, None), ('bn_fold_partials', {4: 0}, None),
    ('bn_fwd_partials', {15: None}, None), ('bn_fwd_partials', {4: 12}, None), ('bn_fwd_partials', {11: 3}, None),
    ('bn_fwd_partials', {17: 0}, 'partial rows'), ('bn_fwd_partials', {17: 5000}, 'partial rows'),
    ('bn_fwd_partials', {18: 0}, None), ('bn_fwd_partials', {18: 3}, None),
    ('bn_coef', {15: None}, None), ('bn_coef', {1: 12}, None), ('bn_coef', {13: 5000}, 'partial rows'),
    ('bn_coef', {14: 0}, None), ('bn_coef', {14: 3}, None), ('bn_coef', {0: 0}, None),
    ('bn_fwd_drop_add', {17: None}, None), ('bn_fwd_drop_add', {4: 12}, None), ('bn_fwd_drop_add', {18: 0}, None),
    ('bn_fwd_drop_add', {18: 5}, None), ('bn_fwd_drop_add', {19: 0.0}, None),
    ('bn_fwd_drop_add', {16: 5000}, None), ('bn_fwd_drop_add', {14: None, 23: None}, None),
    ('bn_fwd_drop_add', {3: 1 << 31, 18: 1}, None),
    ('bn_bwd_scaled', {12: None}, None), ('bn_bwd_scaled', {5: 12}, None), ('bn_bwd_scaled', {13: 0}, None),
    ('bn_bwd_scaled', {13: 5}, None),
    ('bn_bwd_se', {13: None}, None), ('bn_bwd_se', {5: 12}, None), ('bn_bwd_se', {10: 3}, None),
    ('bn_bwd_se', {15: 0}, None), ('bn_bwd_se', {15: 5}, None),
    ('bn_bwd_partials', {15: None}, None), ('bn_bwd_partials', {5: 12}, None), ('bn_bwd_partials', {10: 3}, None),
    ('bn_bwd_partials', {13: P, 14: 16, 10: 2}, None), ('bn_bwd_partials', {16: 70000}, 'partial rows'),
    ('bn_bwd_partials', {16: 0}, 'partial rows'), ('bn_bwd_partials', {13: P, 14: 0}, None),
    ('bn_bwd_partials', {17: 0}, 'groups'), ('bn_bwd_partials', {17: 3}, 'groups'),
    ('bn_bwd_partials', {13: P, 14: 16, 17: 2}, 'groups'),
    ('bn_bwd_reduce', {11: None}, None), ('bn_bwd_reduce', {4: 12}, None), ('bn_bwd_reduce', {9: 3}, None),
    ('bn_bwd_reduce', {10: 0}, None), ('bn_bwd_reduce', {10: 3}, None),
    ('bn_bwd', {15: None}, None), ('bn_bwd', {5: 12}, None), ('bn_bwd', {10: 3}, None), ('bn_bwd', {14: 0}, None),
    ('bn_bwd', {14: 3}, None),
    ('bn_act_se_squeeze', {19: None}, None), ('bn_act_se_squeeze', {5: 12}, None),
    ('bn_act_se_squeeze', {12: 3}, None), ('bn_act_se_squeeze', {4: 0}, None),
    ('dwconv3x3_fwd', {0: None}, None), ('dwconv3x3_fwd', {6: 12}, None), ('dwconv3x3_fwd', {7: 3}, None),
    ('dwconv3x3_fwd', {9: 7}, None),
    ('dwconv3x3_bwd_data', {2: None}, None), ('dwconv3x3_bwd_data', {6: 12}, None),
    ('dwconv3x3_bwd_data', {7: 3}, None),
    ('dwconv3x3_bwd_weight', {11: None}, None), ('dwconv3x3_bwd_weight', {7: 12}, None),
    ('dwconv3x3_bwd_weight', {8: 3}, None),
    ('dwconv3x3_fwd_bn', {9: None}, None), ('dwconv3x3_fwd_bn', {6: 12}, 'not supported'),
    ('dwconv3x3_fwd_bn', {7: 3}, 'not supported'), ('dwconv3x3_fwd_bn', {3: 0}, 'not supported'),
    ('dwconv3x3_bwd_data_bn', {7: None}, None), ('dwconv3x3_bwd_data_bn', {12: 3}, None),
    ('dwconv3x3_bwd_data_bn', {6: 12}, 'not supported'), ('dwconv3x3_bwd_data_bn', {4: 0}, 'not supported'),
    ('dwconv3x3_bwd_fused', {17: None}, None), ('dwconv3x3_bwd_fused', {15: 3}, None),
    ('dwconv3x3_bwd_fused', {9: 12}, 'not supported'), ('dwconv3x3_bwd_fused', {7: 0}, 'not supported'),
    ('dwconv3x3_bwd_fused_se', {18: None}, None), ('dwconv3x3_bwd_fused_se', {23: 3}, None),
    ('dwconv3x3_bwd_fused_se', {15: 3}, None), ('dwconv3x3_bwd_fused_se', {9: 12}, 'not supported'),
    ('dwconv3x3_bwd_fused_se', {6: 0}, 'not supported'),
    ('se_reduce', {0: None}, None), ('se_reduce', {5: 12}, None), ('se_reduce', {4: 0}, None),
    ('se_reduce', {2: 7}, None),
    ('se_scale', {2: None}, None), ('se_scale', {7: 12}, None), ('se_scale', {6: 0}, None),
    ('scale_add', {3: None}, None), ('scale_add', {6: 12}, None), ('scale_add', {2: 7}, None),
    ('scale_add_drop', {1: None}, None), ('scale_add_drop', {9: 12}, None), ('scale_add_drop', {3: 0.0}, None),
    ('se_mlp_fwd', {0: None}, None), ('se_mlp_fwd', {9: 0}, None), ('se_mlp_fwd', {7: 0}, None),
    ('se_mlp_bwd', {0: None}, None), ('se_mlp_bwd', {14: 0}, None), ('se_mlp_bwd', {14: 8193}, None),
    ('se_squeeze_mlp_fwd', {0: None}, None), ('se_squeeze_mlp_fwd', {4: 12}, None),
    ('se_squeeze_mlp_fwd', {3: 0}, None), ('se_squeeze_mlp_fwd', {9: 0}, None),
    ('se_forward', {13: None}, None), ('se_forward', {4: 12}, None), ('se_forward', {3: 0}, None),
    ('se_forward', {3: 1 << 30}, None),
    ('se_gate_excite', {0: None}, None), ('se_gate_excite', {8: 12}, None), ('se_gate_excite', {7: 0}, None),
    ('se_squeeze_mlp_bwd', {0: None}, None), ('se_squeeze_mlp_bwd', {5: 12}, None),
    ('se_squeeze_mlp_bwd', {4: 0}, None),
    ('bn_se_bwd_dx', {14: None}, None), ('bn_se_bwd_dx', {6: 12}, None), ('bn_se_bwd_dx', {11: 3}, None),
    ('bn_se_bwd_dx', {5: 0}, None), ('bn_se_bwd_dx', {6: 4104}, None),
    ('bn_se_bwd', {1: None}, None), ('bn_se_bwd', {7: 12}, None), ('bn_se_bwd', {12: 3}, None),
    ('bn_se_bwd', {6: 0}, None), ('bn_se_bwd', {7: 4104}, None), ('bn_se_bwd', {20: 0}, None),
    ('maxpool2_fwd', {2: None}, None), ('maxpool2_fwd', {7: 12}, None), ('maxpool2_fwd', {5: 1}, None),
    ('maxpool2_bwd', {0: None}, None), ('maxpool2_bwd', {7: 12}, None), ('maxpool2_bwd', {3: 7}, None),
]


def _reject(entry, bad):
    from ewvit import _lib
    lib = _lib.load()
    args = list(GOOD[entry])
    assert len(args) == len(_lib.SIGNATURES['ewvit_' + entry])
    for i, v in bad.items():
        args[i] = v
    rc = getattr(lib, 'ewvit_' + entry)(*args)
    return rc, lib.ewvit_last_error().decode()


def _case_id(case):
    entry, bad, _ = case
    return entry + ''.join('-%d=%s' % (i, 'ptr' if isinstance(v, ctypes.c_void_p) else v) for i, v in bad.items())


@pytest.mark.parametrize('entry,bad,word', REJECTED, ids=[_case_id(c) for c in REJECTED])
def test_block_entry_points_reject_bad_arguments(entry, bad, word):
    rc, msg = _reject(entry, bad)
    assert rc == 1000, (rc, msg)
    assert msg.startswith(entry + ':'), msg
    if word:
        assert word in msg, msg


def test_every_block_entry_point_has_a_rejected_call():
    assert {e for e, _, _ in REJECTED} == set(GOOD)


def test_partial_row_limits_differ_by_entry():
    """5000 partial rows: over the forward-partials forms' limit (4096), within ewvit_bn_bwd_partials'
    (65535) — that call gets past the row check to the next rejection (groups), and with no rows
    (M = 0) it has nothing to launch and succeeds."""
    rc, msg = _reject('bn_fwd_partials', {17: 5000})
    assert rc == 1000 and 'partial rows' in msg
    rc, msg = _reject('bn_coef', {13: 5000})
    assert rc == 1000 and 'partial rows' in msg
    rc, msg = _reject('bn_fwd_drop_add', {16: 5000})
    assert rc == 1000 and msg.startswith('bn_fwd_drop_add:')
    rc, msg = _reject('bn_bwd_partials', {16: 5000, 17: 0})
    assert rc == 1000 and 'groups' in msg and 'partial rows' not in msg
    rc, msg = _reject('bn_bwd_partials', {16: 5000, 4: 0})
    assert rc == 0, msg
    rc, msg = _reject('bn_bwd_partials', {16: 65536})
    assert rc == 1000 and 'partial rows' in msg
    rc, msg = _reject('bn_fwd_partials', {17: 4096, 18: 0})       # 4096 rows pass; the groups do not
    assert rc == 1000 and 'partial rows' not in msg


# (query, arguments, the value the library answered before the host dispatch was deduplicated)
QUERY_VALUES = [
    ('ewvit_bn_workspace', (75, 8, 1), 96),
    ('ewvit_bn_workspace', (75, 72, 3), 2592),
    ('ewvit_bn_workspace', (6272, 960, 1), 96000),
    ('ewvit_bn_workspace', (150528, 64, 3), 151296),
    ('ewvit_bn_workspace', (100, 16, 0), 192),
    ('ewvit_bn_bwd_reduce_rows', (75, 8, 1), 1),
    ('ewvit_bn_bwd_reduce_rows', (75, 72, 3), 1),
    ('ewvit_bn_bwd_reduce_rows', (6272, 960, 1), 12),
    ('ewvit_bn_bwd_reduce_rows', (150528, 64, 3), 98),
    ('ewvit_bn_bwd_reduce_rows', (75, 12, 1), 0),
    ('ewvit_bn_bwd_reduce_rows', (75, 8, 2), 0),
    ('ewvit_dwconv3x3_bn_rows', (2, 5, 5, 8, 1, 0), 1),
    ('ewvit_dwconv3x3_bn_rows', (2, 5, 5, 72, 2, 0), 1),
    ('ewvit_dwconv3x3_bn_rows', (16, 14, 14, 960, 1, 1), 7),
    ('ewvit_dwconv3x3_bn_rows', (2, 5, 5, 72, 2, 1), 0),
    ('ewvit_dwconv3x3_bn_rows', (2, 5, 5, 12, 1, 0), 0),
    ('ewvit_dwconv3x3_bn_rows', (2, 5, 5, 8, 3, 0), 0),
    ('ewvit_dwconv3x3_bwd_weight_workspace', (2, 5, 5, 8, 1, 1), 288),
    ('ewvit_dwconv3x3_bwd_weight_workspace', (2, 5, 5, 72, 2, 1), 2592),
    ('ewvit_dwconv3x3_bwd_weight_workspace', (16, 14, 14, 960, 1, 1), 1935360),
    ('ewvit_dwconv3x3_bwd_weight_workspace', (8, 28, 28, 256, 2, 1), 64512),
    ('ewvit_dwconv3x3_bwd_fused_workspace', (2, 5, 5, 8), 288),
    ('ewvit_dwconv3x3_bwd_fused_workspace', (2, 5, 5, 72), 2592),
    ('ewvit_dwconv3x3_bwd_fused_workspace', (16, 14, 14, 960), 241920),
    ('ewvit_se_reduce_workspace', (3, 9, 72), 864),
    ('ewvit_se_reduce_workspace', (2, 1024, 64), 2048),
    ('ewvit_se_reduce_workspace', (16, 196, 960), 184320),
    ('ewvit_se_mlp_fwd_workspace', (3, 72, 6), 144),
    ('ewvit_se_mlp_fwd_workspace', (16, 960, 40), 38400),
    ('ewvit_se_mlp_bwd_workspace', (3, 72, 6), 1080),
    ('ewvit_se_mlp_bwd_workspace', (16, 960, 40), 102400),
    ('ewvit_bn_se_bwd_workspace', (3, 72, 6), 5112),
    ('ewvit_bn_se_bwd_workspace', (16, 960, 40), 355840),
    ('ewvit_bn_se_bwd_row_offset', (3, 72, 6), 1134),
    ('ewvit_bn_se_bwd_row_offset', (16, 960, 40), 87040),
]


@pytest.mark.parametrize('name,args,want', QUERY_VALUES, ids=[f'{n}{a}' for n, a, _ in QUERY_VALUES])
def test_size_queries_keep_their_values(name, args, want):
    from ewvit import _lib
    assert getattr(_lib.load(), name)(*args) == want


def test_ops_refuse_cpu_tensors():
    import torch
    import ewvit
    x = torch.randn(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ewvit.dwt_haar(x, 1)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ewvit.linear(torch.randn(2, 4), torch.randn(3, 4))

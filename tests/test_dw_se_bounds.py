"""
CPU checks of the depthwise / SE sweep in tests/test_gpu_dw_se.py: its parameter table reaches all 24 depthwise kernel instances
and every activation code of each, its float64 depthwise restatement agrees with F.conv2d(groups=C), and its bounds are tight
enough to fail - the float64 result of a plausible kernel bug violates the bound of the correct result somewhere.
"""

import pytest
import torch
import torch.nn.functional as F

from test_gpu_dw_se import (DW_INSTANCES, FAST_CODES, GENERAL_CODES, NONE, RELU, SIGMOID, HSIGMOID, SWISH, U32, _iid, act64,
                            bn_fold64, dw_cases, dw_operands, dw_out_hw, dw_ref, fc_ref, is_fast, mean_ref, out_bound, scale_ref,
                            se_mlp, taps_of)


def _table():
    return [(ks, s, is_fast(act, post), dt, act, post, with_res)
            for ks in (3, 5) for s in (1, 2) for fast in (True, False) for dt in ("fp32", "bf16", "fp16")
            for (N, H, W, C, pad4, act, post, with_res) in dw_cases(ks, s, fast)]


def test_depthwise_table_reaches_all_24_instances():
    """FAST index of the kDw table: act <= RELU6 and post_act <= RELU6 -> FAST; {3, 5} x stride {1, 2} x FAST x 3 dtypes"""
    reached = {(ks, s, fast, dt) for (ks, s, fast, dt, _, _, _) in _table()}
    assert reached == set(DW_INSTANCES) and len(reached) == 24


def test_depthwise_table_covers_every_activation_of_each_class():
    for inst in DW_INSTANCES:
        rows = [r for r in _table() if r[:4] == inst]
        codes = FAST_CODES if inst[2] else GENERAL_CODES
        assert {r[4] for r in rows} >= set(codes), _iid(inst)
        if inst[1] == 1:
            res_rows = [r for r in rows if r[6]]
            assert res_rows, _iid(inst)
            assert {r[5] for r in res_rows} >= set(codes) - {NONE}, _iid(inst)
            if not inst[2]:           # a general post_act behind a clamp act forces the general instance
                assert any(r[4] <= 2 for r in res_rows), _iid(inst)


@pytest.mark.parametrize("ks,s,pad4", [(3, 1, (1, 1, 1, 1)), (3, 2, (0, 1, 0, 1)), (5, 1, (1, 3, 3, 1)), (5, 2, (1, 2, 1, 2)),
                                       (5, 1, (2, 2, 2, 2))])
def test_float64_restatement_matches_conv2d(ks, s, pad4):
    x, w, bn, _ = dw_operands(2, 11, 9, 16, ks, "fp32", seed=3)
    sc, sh = bn_fold64(bn)
    ref, _ = dw_ref(x, taps_of(w, "fp32"), sc, sh, ks, s, pad4, NONE)
    l, r, t, b = pad4
    want = F.conv2d(F.pad(x.permute(0, 3, 1, 2).double(), (l, r, t, b)), w.double(), stride=s, groups=16)
    want = want * sc[:, None, None] + sh[:, None, None]
    assert ref.shape == want.permute(0, 2, 3, 1).shape
    assert torch.allclose(ref, want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def _first_tall_case(ks, s, fast):
    """the first table case of an instance class whose output has more than 4 rows and columns (room for the bug models)"""
    for case in dw_cases(ks, s, fast):
        N, H, W, C, pad4 = case[:5]
        Ho, Wo = dw_out_hw(H, W, ks, s, pad4)
        if Ho > 4 and Wo > 4 and N * H * W * C <= 200000:
            return case
    raise AssertionError("no case with room for the bug models")


def _shift(x, dim):
    """x moved by one step along `dim` (the window reads one input row / column further on), zero filled"""
    idx = torch.arange(1, x.shape[dim])
    return F.pad(x.index_select(dim, idx), (0, 0) * (x.dim() - 1 - dim) + (0, 1))


@pytest.mark.parametrize("inst", DW_INSTANCES, ids=[_iid(p) for p in DW_INSTANCES])
def test_depthwise_bug_models_violate_the_bound(inst):
    ks, s, fast, dtype = inst
    N, H, W, C, pad4, act, post, with_res = _first_tall_case(ks, s, fast)
    Ho, Wo = dw_out_hw(H, W, ks, s, pad4)
    x, w, bn, res = dw_operands(N, H, W, C, ks, dtype, seed=11, Ho=Ho, Wo=Wo, with_res=with_res)
    taps = taps_of(w, dtype)
    sc, sh = [t.float() for t in bn_fold64(bn)]

    def run(xx=x, tt=taps):
        return dw_ref(xx, tt, sc, sh, ks, s, pad4, act, res, post)[0]
    ref, err = dw_ref(x, taps, sc, sh, ks, s, pad4, act, res, post)
    bound = out_bound(ref, err, dtype)

    def violates(bug):
        return bool(((bug - ref).abs() > bound).any())
    for k in (0, ks * ks // 2, ks * ks - 1):                  # one tap dropped
        dropped = taps.clone()
        dropped[k] = 0
        assert violates(run(tt=dropped)), "dropped tap {}".format(k)
    assert violates(run(xx=_shift(x, 2))), "window shifted by one column"
    assert violates(run(xx=_shift(x, 1))), "window shifted by one row"
    dup = ref.clone()                                         # strips of 4 rows: each strip's first row repeats the row before it
    dup[:, 4::4] = ref[:, 3:Ho - 1:4][:, :dup[:, 4::4].shape[1]]
    assert violates(dup), "rows duplicated across a strip boundary"


def test_squeeze_bug_model_violates_the_bound():
    x = torch.randn((3, 7, 7, 72), generator=torch.Generator().manual_seed(1)) + 0.5
    ref, err = mean_ref(x)
    flat = x.view(3, 49, 72)
    assert bool(((flat[:, :48].double().sum(1) / 49 - ref).abs() > err).any()), "one pixel dropped"
    assert bool(((ref.roll(1, 0) - ref).abs() > err).any()), "another image's mean"


def test_excite_bug_models_violate_the_bound():
    for (N, C, M, ma, oa) in [(9, 1032, 120, RELU, SIGMOID), (7, 72, 18, RELU, HSIGMOID), (8, 1024, 20, SWISH, SIGMOID)]:
        g = torch.Generator().manual_seed(C)
        mean = torch.randn(N, C, generator=g)
        w1, b1, w2, b2 = se_mlp(C, M, C + M)
        mid, pre1, e_mid = fc_ref(mean, w1, b1, ma)
        gate, _, e_gate = fc_ref(mid, w2, b2, oa, e_x=e_mid)
        skipped, _, _ = fc_ref(pre1, w2, b2, oa)               # mid activation skipped
        assert bool(((skipped - gate).abs() > e_gate).any()), (N, C, M)
        assert bool(((mid.roll(1, 0) - mid).abs() > e_mid).any()), "another image's mid"
        short, _, _ = fc_ref(mean[:, :-4], w1[:, :-4], b1, ma)  # the K tail dropped
        assert bool(((short - mid).abs() > e_mid).any()), "K tail dropped"


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_se_scale_bug_models_violate_the_bound(dtype):
    g = torch.Generator().manual_seed(4)
    x = torch.randn((3, 7, 7, 72), generator=g)
    res = torch.randn((3, 7, 7, 72), generator=g)
    gate = torch.rand((3, 72), generator=g)
    for post in (NONE, RELU, SWISH, HSIGMOID):
        ref, err = scale_ref(x, gate, res, post)
        bound = out_bound(ref, err, dtype)
        bug, _ = scale_ref(x, gate.roll(1, 0), res, post)       # another image's gate
        assert bool(((bug - ref).abs() > bound).any()), post
        bug, _ = scale_ref(x, gate, None, post)                  # residual ignored
        assert bool(((bug - ref).abs() > bound).any()), post


def test_activation_references_and_error_terms():
    v = torch.linspace(-8, 8, 161, dtype=torch.float64)
    assert torch.equal(act64(v, SIGMOID), torch.sigmoid(v))
    assert float((act64(v, HSIGMOID) - torch.clamp(v + 3, 0, 6) / 6).abs().max()) == 0.0
    from test_gpu_dw_se import LIP, act_err
    for code, lip in LIP.items():                            # the Lipschitz constants hold on a fine grid
        d = (act64(v[1:], code) - act64(v[:-1], code)).abs() / (v[1:] - v[:-1])
        assert float(d.max()) <= lip + 1e-12, code
        assert bool((act_err(v, torch.zeros_like(v), code) >= 0).all())
    assert U32 == 2.0 ** -24

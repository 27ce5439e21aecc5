"""BatchNorm re-estimation, host side: the float64 definition of tests/_bn_estimate.py against what
torch does (reset_running_stats(), momentum = None, train-mode forwards) on the float64 copy of the
oracle network, the pooled estimator against two-pass moments of the concatenated rows, and the
table layout / argument checks of the package that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import _bn_estimate as E
import cilrs_oracle as O

H, W = 40, 120
SIZES_SEEDS = ((3, 10), (5, 11), (2, 12))


@pytest.fixture(scope="module")
def oracle64():
    return O.build_oracle(1).double()


@pytest.fixture(scope="module")
def batches64():
    return [tuple(t.double() if t.is_floating_point() else t
                  for t in O.synthetic_batch(b, seed=s, h=H, w=W)[:3]) for b, s in SIZES_SEEDS]


@pytest.fixture(scope="module")
def stats64(oracle64, batches64):
    return E.batch_stats(oracle64, batches64)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_batch_mean_definition_is_torchs_momentum_none(oracle64, batches64, stats64):
    """all 36 layers: running_mean, running_var to 1e-12 relative, num_batches_tracked exactly"""
    got = E.finalize(E.table_of(stats64), "batch_mean")
    ref = E.torch_update_bn(oracle64, batches64)
    assert len(ref) == 36 and set(got) == set(ref)
    worst_m = worst_v = 0.0
    for name, (rm, rv, nbt) in ref.items():
        assert got[name][2] == nbt == 3
        worst_m = max(worst_m, _rel(got[name][0], rm))
        worst_v = max(worst_v, _rel(got[name][1], rv))
    print(f"BN-EST host batch_mean vs torch momentum=None: mean {worst_m:.3e} var {worst_v:.3e}")
    assert worst_m <= 1e-12 and worst_v <= 1e-12
    # the smallest layer of these shapes has 16 rows in the 2-frame batch
    assert min(M for per in stats64.values() for M, _m, _v in per) == 16


def test_pooled_definition_is_the_two_pass_moments_of_all_rows_of_the_stem(oracle64, batches64,
                                                                           stats64):
    got = E.finalize(E.table_of(stats64), "pooled")
    with torch.no_grad():
        y = oracle64.visual_encoder[0](torch.cat([b[0] for b in batches64]))      # pre-BN rows
    rows = y.permute(0, 2, 3, 1).reshape(-1, y.size(1)).numpy()
    mean = rows.mean(0)
    var = ((rows - mean) ** 2).sum(0) / (rows.shape[0] - 1)
    rm, rv, nbt = got["visual_encoder.1"]
    print(f"BN-EST host pooled vs two-pass: mean {_rel(rm, mean):.3e} var {_rel(rv, var):.3e}")
    assert nbt == 3
    assert _rel(rm, mean) <= 1e-12 and _rel(rv, var) <= 1e-12


def test_pooled_stem_does_not_depend_on_the_batching(oracle64, batches64):
    one = torch.cat([batches64[1][0], batches64[2][0]])
    joined = (one, torch.cat([batches64[1][1], batches64[2][1]]),
              torch.cat([batches64[1][2], batches64[2][2]]))
    a = E.reestimate(oracle64, batches64[1:], "pooled")["visual_encoder.1"]
    b = E.reestimate(oracle64, [joined], "pooled")["visual_encoder.1"]
    assert _rel(a[0], b[0]) <= 1e-12 and _rel(a[1], b[1]) <= 1e-12
    assert (a[2], b[2]) == (2, 1)


def test_the_definition_leaves_the_callers_model_alone(oracle64, batches64):
    before = {k: v.clone() for k, v in oracle64.state_dict().items()}
    E.reestimate(oracle64, batches64[:1])
    E.torch_update_bn(oracle64, batches64[:1])
    assert all(torch.equal(v, before[k]) for k, v in oracle64.state_dict().items())


# ---- the package, without a device --------------------------------------------------------------
@pytest.mark.parametrize("variant,nbn", [(0, 36), (1, 53)])
def test_table_layout_covers_the_table_without_gaps(variant, nbn):
    from cilrs_mi355 import _lib as L
    from cilrs_mi355.bn_estimate import stats_layout
    lay = stats_layout(variant)
    assert len(lay) == nbn
    total = L.lib().cilrs_variant_bn_stats_doubles(variant)
    want = 2 * nbn
    for j, (_name, ch, head, sums) in enumerate(lay):
        assert head == 2 * j and sums == want
        want += 4 * ch
    assert want == total
    # names and channel counts are those of the buffer layout
    from cilrs_mi355.engine import _layout
    assert [(n, c) for n, c, _h, _s in lay] == [(n, c) for n, c, _rm, _rv in _layout(variant)[1]]


def test_layout_names_are_the_oracles_batchnorm_modules():
    from cilrs_mi355.bn_estimate import stats_layout
    assert sorted(n for n, *_ in stats_layout(0)) == sorted(n for n, _ in E.bn_layers(O.build_oracle(0)))


def test_layout_query_refuses_bad_indices():
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    assert lib.cilrs_variant_bn_stats_doubles(99) == 0
    ch, a, b = L.i32(), L.sz(), L.sz()
    assert lib.cilrs_variant_bn_stats_info(0, 36, C.byref(ch), C.byref(a), C.byref(b)) != 0
    assert lib.cilrs_variant_bn_stats_info(0, -1, C.byref(ch), C.byref(a), C.byref(b)) != 0
    assert lib.cilrs_variant_bn_stats_info(7, 0, C.byref(ch), C.byref(a), C.byref(b)) != 0


def test_estimator_names():
    from cilrs_mi355.bn_estimate import ESTIMATORS, estimator_code
    assert ESTIMATORS == ("batch_mean", "pooled")
    assert [estimator_code(e) for e in ESTIMATORS] == [0, 1]
    for bad in ("mean", None, 0, ""):
        with pytest.raises(ValueError):
            estimator_code(bad)


def test_batches_may_be_tensors_or_tuples_starting_with_one():
    from cilrs_mi355.bn_estimate import _images_of
    x = torch.zeros(2, 3, 4, 4)
    assert _images_of(x) is x and _images_of((x, 1, 2, 3)) is x and _images_of([x]) is x
    with pytest.raises(TypeError):
        _images_of(("frames.npy", 1))


def test_null_arguments_are_refused_before_any_device_call():
    """no device here: reaching a launch would fail differently (or crash)"""
    from cilrs_mi355 import _lib as L
    lib = L.lib()
    buf = (C.c_double * 8)()
    assert lib.cilrs_bn_stats_finalize(0, None, 0, buf, buf, None) != 0
    assert b"NULL" in lib.cilrs_last_error()
    assert lib.cilrs_bn_stats_finalize(0, buf, 2, buf, buf, None) != 0
    assert b"estimator" in lib.cilrs_last_error()
    assert lib.cilrs_bn_stats_finalize(9, buf, 0, buf, buf, None) != 0
    assert lib.cilrs_bn_train_stats(None, 8, 64, buf, buf, None) != 0
    assert lib.cilrs_bn_train_stats(buf, 1, 64, buf, buf, None) != 0
    assert b"M >= 2" in lib.cilrs_last_error()
    assert lib.cilrs_bn_train_stats(buf, 8, 60, buf, buf, None) != 0

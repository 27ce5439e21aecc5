"""Host checks of oracle/infer16_emulation.py, the CPU definition of the 16-bit inference mode: with
the rounding switched off it is the fp32 oracle (the fold and the block wiring are right before any
rounding enters), with it on it stays inside the tolerances the end-to-end GPU tests use, and the
distance between two realisations of the same rounded computation -- the yardstick of the
end-to-end step of tests/test_infer16_gpu.py -- is printed."""
import pytest
import torch

import cilrs_oracle as O
import infer16_emulation as E

TOL_OUT = 1e-4
TOL_F16 = TOL_BF16 = 1e-2           # tests/test_model_gpu.py


def _oracle(net):
    if net == "resnet34":
        return O.build_oracle(0).eval()
    import resnet50_oracle as R
    return R.build_oracle50(0).eval()


@pytest.mark.parametrize("net", ["resnet34", "resnet50"])
def test_emulation_without_rounding_is_the_fp32_oracle(net):
    orc = _oracle(net)
    img, spd, cmd = O.synthetic_batch(3, seed=123)[:3]
    with torch.no_grad():
        oc, os_ = orc(img, spd, cmd)
    for T in (torch.float32, torch.float64):
        c, s = E.forward(orc, img, spd, cmd, T, acc=T)
        err = max(float((c - oc).abs().max()), float((s - os_).abs().max()))
        print(f"{net} unrounded emulation ({T}) vs fp32 oracle: {err:.3e}")
        assert err <= TOL_OUT


@pytest.mark.parametrize("net", ["resnet34", "resnet50"])
@pytest.mark.parametrize("T,tol", [(torch.float16, TOL_F16), (torch.bfloat16, TOL_BF16)])
def test_rounded_emulation_is_close_to_fp32_and_another_arithmetic(net, T, tol):
    orc = _oracle(net)
    img, spd, cmd = O.synthetic_batch(3, seed=123)[:3]
    with torch.no_grad():
        oc, os_ = orc(img, spd, cmd)
    c, s = E.forward(orc, img, spd, cmd, T)
    err = max(float((c - oc).abs().max()), float((s - os_).abs().max()))
    print(f"{net} {T} emulation vs fp32 oracle: {err:.3e}")
    assert 0 < err <= tol


@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,seed", [(3, 123), (6, 7)])
def test_self_distance_of_two_realisations_is_reported(T, B, seed):
    """fp32- and float64-accumulating realisations of the SAME rounded computation, on the pooled
    features: a sum that differs in the last fp32 bit lands on the other 16-bit neighbour now and
    then and the difference propagates, so they are not equal -- and not far apart either."""
    orc = _oracle("resnet34")
    img = O.synthetic_batch(B, seed=seed)[0]
    f32 = E.features(orc, img, T, torch.float32).double()
    f64 = E.features(orc, img, T, torch.float64)
    with torch.no_grad():
        fo = orc.visual_encoder(img).double()
    d = f32 - f64
    do = f64 - fo
    print(f"ResNet-34 {T} B={B}: |feature| max {float(f64.abs().max()):.2f}; emu32 - emu64 max "
          f"{float(d.abs().max()):.3e} rms {float(d.pow(2).mean().sqrt()):.3e}; emu64 - fp32 oracle "
          f"max {float(do.abs().max()):.3e} rms {float(do.pow(2).mean().sqrt()):.3e}")
    assert torch.isfinite(f32).all() and torch.isfinite(f64).all()
    assert 0 < float(d.abs().max()) < float(f64.abs().max()) * 2.0 ** -4


@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16])
def test_direct_rounding_of_float64(T):
    """round_to on float64 is ONE rounding: exact on values of T, ties to even, and differs from
    rounding through fp32 exactly where that rounds twice."""
    p = {torch.float16: 11, torch.bfloat16: 8}[T]
    g = torch.Generator().manual_seed(5)
    v = torch.randn(4096, generator=g).to(T)
    assert torch.equal(E.round_to(v.double(), T), v.double())
    one = torch.tensor([1.0], dtype=torch.float64)
    ulp = 2.0 ** (1 - p)
    assert float(E.round_to(one + 0.5 * ulp, T)) == 1.0                      # tie -> even
    assert float(E.round_to(one + 1.5 * ulp, T)) == 1.0 + 2 * ulp            # tie -> even
    x = one + 0.5 * ulp + 2.0 ** -40                                         # just above a tie
    assert float(E.round_to(x, T)) == 1.0 + ulp
    assert float(x.float().to(T)) == 1.0                                     # through fp32: twice
    assert float(E.half_spacing(torch.tensor([1.5], dtype=torch.float64), T)) == 0.5 * ulp
    assert float(E.half_spacing(torch.tensor([0.0], dtype=torch.float64), T)) == 0.0
    if T == torch.float16:                                                   # subnormal spacing 2^-24
        assert float(E.round_to(torch.tensor([2.0 ** -25 * 1.01], dtype=torch.float64), T)) == 2.0 ** -24


def test_perturbed_statistics_keep_the_network_usable():
    orc = _oracle("resnet34")
    sd = E.perturbed_state_dict(orc.state_dict(), 0)
    assert float(sd["visual_encoder.1.running_var"].min()) >= 1e-3
    assert float(sd["visual_encoder.1.running_var"].max()) <= 1e2
    assert (sd["visual_encoder.4.0.bn1.weight"] < 0).any() and (sd["visual_encoder.4.0.bn1.weight"] > 0).any()
    orc.load_state_dict(sd)
    img = O.synthetic_batch(2, seed=3)[0]
    with torch.no_grad():
        f = orc.visual_encoder(img)
    print(f"perturbed-statistics ResNet-34: |feature| max {float(f.abs().max()):.2f}")
    assert torch.isfinite(f).all() and 0.05 < float(f.abs().max()) < 100.0

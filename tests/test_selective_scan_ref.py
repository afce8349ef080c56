"""The sequential restatement of the selective scan (tests/selective_scan_ref.py) against answers worked out without it."""
import torch
import torch.nn.functional as F

import selective_scan_ref as R

B_, D_, L_ = 2, 5, 37


def test_zero_A_is_a_running_sum():
    s = R.structured(B_, D_, L_)
    out = R.selective_scan(s["u"], s["dt"], torch.zeros(D_, R.N, dtype=torch.float64), s["B"], s["C"])
    want = R.running_sum_answer(s["dt"], s["B"], s["C"], s["u"])
    assert R.norm_err(out, want) < 1e-13
    # swapping B with C, or reversing time, is a different answer: the inputs tell them apart
    assert R.norm_err(R.selective_scan(s["u"], s["dt"], torch.zeros(D_, R.N, dtype=torch.float64), s["C"], s["B"]), want) > 1e-2
    assert R.norm_err(out.flip(-1), want) > 1e-2


def test_zero_delta_leaves_the_skip_path():
    s = R.structured(B_, D_, L_)
    out, last = R.selective_scan(s["u"], torch.zeros_like(s["dt"]), s["A"], s["B"], s["C"], s["D"], z=s["z"], return_last_state=True)
    assert torch.equal(out, s["D"][None, :, None] * s["u"] * F.silu(s["z"]))
    assert torch.equal(last, torch.zeros(B_, D_, R.N, dtype=torch.float64))


def test_impulse_decays_in_closed_form():
    s = R.structured(B_, D_, L_)
    k = [3, 20]
    amp = 1.0 + 0.25 * torch.arange(B_ * D_, dtype=torch.float64).reshape(B_, D_)
    u = torch.zeros(B_, D_, L_, dtype=torch.float64)
    for b in range(B_):
        u[b, :, k[b]] = amp[b]
    out, last = R.selective_scan(u, s["dt"], s["A"], s["B"], s["C"], return_last_state=True)
    want = R.impulse_answer(s["dt"], s["A"], s["B"], s["C"], amp, k)
    assert R.norm_err(out, want) < 1e-13
    assert float(out[0, :, :3].abs().max()) == 0.0 and float(out[1, :, :20].abs().max()) == 0.0
    decay = s["dt"][0, :, 4:].sum(-1)
    want_last = s["dt"][0, :, 3, None] * s["B"][0, None, :, 3] * amp[0, :, None] * torch.exp(s["A"] * decay[:, None])
    assert R.norm_err(last[0], want_last) < 1e-13


def test_softplus_bias_groups_and_gate():
    """Group g(d) = d // (D / G), the bias is added before softplus, softplus is the identity above 20."""
    t, _ = R.make_inputs(2, 6, 9, groups=2, seed=3)
    t["delta"][0, 0, 0] = 25.0
    out = R.selective_scan(**t, delta_softplus=True)
    dt = F.softplus(t["delta"] + t["delta_bias"][None, :, None])
    assert float(dt[0, 0, 0]) == 25.0 + float(t["delta_bias"][0])
    for d in (0, 2, 3, 5):
        one = R.selective_scan(t["u"][:, d:d + 1], dt[:, d:d + 1], t["A"][d:d + 1], t["B"][:, d // 3], t["C"][:, d // 3], t["D"][d:d + 1],
                               z=t["z"][:, d:d + 1])
        assert R.norm_err(out[:, d:d + 1], one) < 1e-14


def test_inner_composition_matches_module_form():
    """The composition against nn.Conv1d / nn.Linear written the way Mamba.forward's slow path writes them."""
    torch.manual_seed(0)
    d_model, d_inner, rank, L, width = 8, 16, 2, 11, 4
    conv = torch.nn.Conv1d(d_inner, d_inner, width, groups=d_inner, padding=width - 1).double()
    x_proj = torch.nn.Linear(d_inner, rank + 2 * R.N, bias=False).double()
    dt_proj = torch.nn.Linear(rank, d_inner).double()
    A = -torch.exp(torch.randn(d_inner, R.N, dtype=torch.float64))
    Dp = torch.randn(d_inner, dtype=torch.float64)
    xz = torch.randn(2, 2 * d_inner, L, dtype=torch.float64)
    got = R.mamba_inner_no_out_proj(xz, conv.weight, conv.bias, x_proj.weight, dt_proj.weight, A, Dp, dt_proj.bias)
    x, z = xz.chunk(2, dim=1)
    x = F.silu(conv(x)[..., :L])
    x_dbl = x_proj(x.transpose(1, 2))
    dt, Bm, Cm = torch.split(x_dbl, [rank, R.N, R.N], dim=-1)
    dt = (dt @ dt_proj.weight.t()).transpose(1, 2)
    want = R.selective_scan(x, dt, A, Bm.transpose(1, 2), Cm.transpose(1, 2), Dp, z=z, delta_bias=dt_proj.bias, delta_softplus=True)
    assert R.norm_err(got, want) < 1e-13


def test_yardstick_is_small_and_bar_has_a_floor():
    t, dout = R.make_inputs(2, 5, 65, seed=1)
    _, g64, ys = R.yardstick_case(t, dout, delta_softplus=True)
    assert set(ys) == {"out", *R.GRAD_NAMES}
    assert all(0.0 <= v < 1e-4 for v in ys.values()), ys
    assert R.bar(0.0) == R.FLOOR and R.bar(1e-5) == 4e-5

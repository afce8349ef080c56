"""libunipre3d_selective_scan.so writes every element it owns and nothing else: its entry points called directly, with every pointer
inside a poisoned arena (tests/guarded.py), under two poisons.  Expected values: the module's own wrapper on ordinary tensors, bit for
bit (tests/test_gpu_selective_scan.py holds the wrapper to the fp64 restatement).

  entry point     cases
  u3d_sscan_fwd   (B, D, G, L) = (2, 5, 1, 65): one step past a 64-lane load, an odd channel count;  (2, 6, 2, 129): two groups, one step
  u3d_sscan_bwd   past two loads;  (2, 70, 1, 257): two 64-channel slabs (dB / dC through the partials buffer and the reduce launch) and
                  two passes (two xsave records per row, the second pass one step long);  (1, 3, 3, 5): a row shorter than a wave, one
                  channel per group.  Each with D, z and delta_bias and their three gradients, and with all six NULL.  xsave is passed
                  to the forward at every shape (one record per row where there is one pass; it then equals last_state).  The
                  backward's scratch is a guarded placement, 256-byte aligned.
"""
import numpy as np
import pytest
import torch

from guarded import run_twice, same_bits

pytestmark = pytest.mark.gpu
N = 16


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("B, D, G, L", [(2, 5, 1, 65), (2, 6, 2, 129), (2, 70, 1, 257), (1, 3, 3, 5)])
def test_selective_scan_writes_what_it_owns(B, D, G, L, full):
    from unipre3d_amd import _lib, selective_scan as ss
    lib = ss.load()
    rng = np.random.default_rng(D * 1000 + L)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    cpu = {"u": f(B, D, L), "delta": 0.5 * f(B, D, L), "A": -torch.from_numpy(rng.uniform(0.5, 4.0, (D, N)).astype(np.float32)),
           "Bm": f(B, G, N, L), "Cm": f(B, G, N, L), "dout": f(B, D, L)}
    if full:
        cpu.update(Dv=f(D), z=f(B, D, L), delta_bias=0.1 * f(D))
    npass = -(-L // ss.pass_len(L))
    assert npass == (2 if L == 257 else 1)
    nbytes = int(lib.u3d_sscan_bwd_scratch_bytes(B, D, G, L))

    dev = {k: v.cuda().requires_grad_(k != "dout") for k, v in cpu.items()}
    out, last = ss.selective_scan_fn(dev["u"], dev["delta"], dev["A"], dev["Bm"], dev["Cm"], dev.get("Dv"), dev.get("z"),
                                     dev.get("delta_bias"), delta_softplus=True, return_last_state=True)
    xsave_want = out.grad_fn.saved_tensors[8]
    assert (xsave_want is None) == (npass == 1)
    out.backward(dev["dout"])
    xsave_cpu = None if xsave_want is None else xsave_want.cpu()

    def case(arena):
        t = {k: arena.inp(v, name=k) for k, v in cpu.items()}
        p, g = _lib.ptr, t.get
        o = arena.out((B, D, L), torch.float32, name="out")
        ls = arena.out((B, D, N), torch.float32, name="last_state")
        xs = arena.out((B, D, npass, N), torch.float32, name="xsave")
        st = _lib.stream_ptr(o.device)
        assert lib.u3d_sscan_fwd(p(t["u"]), p(t["delta"]), p(t["A"]), p(t["Bm"]), p(t["Cm"]), p(g("Dv")), p(g("z")), p(g("delta_bias")),
                                 p(o), p(ls), p(xs), B, D, G, N, L, 1, st) == 0
        xs_in = arena.inp(xsave_cpu, name="xsave_in") if npass > 1 else None
        outs = {k: arena.out(cpu[src].shape, torch.float32, name=k)
                for k, src in (("du", "u"), ("ddelta", "u"), ("dA", "A"), ("dB", "Bm"), ("dC", "Cm"))}
        if full:
            outs.update({k: arena.out(cpu[src].shape, torch.float32, name=k) for k, src in (("dD", "Dv"), ("dz", "z"), ("ddelta_bias", "delta_bias"))})
        scratch = arena.out((max(nbytes, 1),), torch.uint8, name="scratch")
        assert scratch.data_ptr() % 256 == 0
        assert lib.u3d_sscan_bwd(p(t["u"]), p(t["delta"]), p(t["A"]), p(t["Bm"]), p(t["Cm"]), p(g("Dv")), p(g("z")), p(g("delta_bias")),
                                 p(t["dout"]), p(xs_in), p(outs["du"]), p(outs["ddelta"]), p(outs["dA"]), p(outs["dB"]), p(outs["dC"]),
                                 p(outs.get("dD")), p(outs.get("dz")), p(outs.get("ddelta_bias")), p(scratch), nbytes,
                                 B, D, G, N, L, 1, st) == 0
        return [o, ls, xs] + list(outs.values())

    run, _ = run_twice(case, "cuda", capacity=64 << 20)
    want = [out.detach(), last, xsave_want if npass > 1 else last.unsqueeze(2)]
    want += [dev[k].grad for k in ("u", "delta", "A", "Bm", "Cm")]
    names = ["out", "last_state", "xsave", "du", "ddelta", "dA", "dB", "dC"]
    if full:
        want += [dev[k].grad for k in ("Dv", "z", "delta_bias")]
        names += ["dD", "dz", "ddelta_bias"]
    assert len(run) == len(want)
    for got, exp, name in zip(run, want, names):
        assert same_bits(got, exp), name

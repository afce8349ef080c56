#!/usr/bin/env python3
"""Generates tests/golden/g24_tokenizer.npz: what the reference's OWN `Encoder` (openpoints/models/backbone/transformer.py and
openpoints/models/Mamba3D/Mamba3D.py, the same text twice, both loaded by path under stub packages, as they are) computes on the CPU in
fp64, with autograd's gradients, for unipre3d_amd/tokenizer.py and tests/tokenizer_ref.py.  The recipe asserts that the two classes give
bit-identical results (in fp32 and in fp64) and records that.  Only inputs and recorded results are stored: the weights, BN affine and
running statistics come from the closed-form recipe tokenizer_ref.weights(C) and the file holds their checksums.

  names, state_keys, classes_bit_identical, weight_checksums (16, 2: sum and sum of |.| in the order PARAMS + RUNNING), C, eps, momentum, nbt0
  {case}_x        fp32 (B, G, n, 3); `strided`: (B, 3, G, n), fed through the transformer's permute(0, 2, 3, 1)
  {case}_dout     fp32 (B, G, C) on a 2^-4 grid
  {case}_out64    fp64 (B, G, C)
  {case}_d{p}64   fp64 gradient of parameter p (the (out, in) shape; dW2, dW3 and dW4 at the flat indices 0, step, 2 step, ... of
                  tokenizer_ref.SUBSET_STEP, the steps coprime to the row lengths; in full the record would be larger than any other), {case}_dx64
  {case}_{rm1,rv1,rm2,rv2}64, {case}_nbt   the running statistics (of the fp64 module) and num_batches_tracked after the step
  {case}_yard_{out,dparams,dx,running}     the yardsticks: the reference's own fp32 run against its fp64 run, max|x - ref| / max|ref|

Cases at C = 40, (B, G, n) = (2, 3, 8): train; eval; padded (the second half of every group repeats its first row, as ball-query padding
does); strided.

With --tolerance it also measures the floors (the fp32 restatement in the kernels' order against the fp64 record, and at every edge shape
against the fp64 restatement) and writes profiles/tokenizer/tolerance.json, keeping the kernels' recorded worst figures if the file
already has them.  --kernel-log FILE alone reads the figures tests/test_gpu_tokenizer.py prints (pytest -s) on an MI355X and records them
as `kernel_worst` in that file."""
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
import tokenizer_ref as TR  # noqa: E402
import make_g19_dense_attention as g19  # noqa: E402
import make_g20_lnp as g20  # noqa: E402

C, SHAPE = 40, (2, 3, 8)


def cases():
    rng = np.random.default_rng(24)
    B, G, n = SHAPE
    out = {}
    for name in TR.CASES:
        x = rng.uniform(-1, 1, (B, G, n, 3)).astype(np.float32)
        if name == "padded":
            x[:, :, n // 2:] = x[:, :, :1]
        if name == "strided":
            x = np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))
        dout = (np.round(rng.uniform(-1, 1, (B, G, C)) * 16) / 16).astype(np.float32)
        out[name] = (x, dout)
    return out


def run(cls, w, x, dout, dtype, training):
    m = cls(C)
    m.load_state_dict(TR.state_dict(w), strict=True)
    m = m.to(dtype)
    m.train(training)
    return TR.reference_run(m, x, dout) + (list(m.state_dict().keys()),)


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    enc_t, enc_m = g19.load_reference().Encoder, g20.load_reference().Encoder
    w = TR.weights(C)
    rec = {"names": np.asarray(TR.CASES), "C": np.int64(C), "eps": np.float64(TR.EPS), "momentum": np.float64(TR.MOMENTUM),
           "nbt0": np.int64(TR.NBT0), "weight_checksums": TR.checksums(w)}
    identical = True
    for name, (x_rec, dout) in cases().items():
        x = np.transpose(x_rec, (0, 2, 3, 1)) if name == "strided" else x_rec
        training = name != "eval"
        res = {}
        for dtype in (torch.float64, torch.float32):
            a = run(enc_t, w, x, dout, dtype, training)        # (x: a numpy view; torch keeps its strides)
            b = run(enc_m, w, x, dout, dtype, training)
            identical &= same(a[0], b[0]) and all(same(a[1][k], b[1][k]) for k in a[1]) and all(same(a[2][k], b[2][k]) for k in a[2])
            assert a[4] == b[4]
            res[dtype] = a
        assert identical, f"{name}: the two reference classes differ"
        o64, g64, r64, nbt, keys = res[torch.float64]
        o32, g32, r32, _, _ = res[torch.float32]
        rec["state_keys"] = np.asarray(keys)
        ref = dict(TR.recorded(g64), out=o64, **r64)
        got = dict(TR.recorded(g32), out=o32, **r32)
        # the fp64 restatement IS the reference's fp64 arithmetic, forward and gradient
        s = TR.forward(x, w, training=training)
        mine = dict(TR.recorded(TR.backward(s, dout)), out=s["out"], **s["running"])
        dm = TR.distances(mine, ref, training)
        assert max(dm.values()) < 1e-11 and s["nbt"] == nbt, (name, dm, s["nbt"], nbt)
        rec.update({f"{name}_x": x_rec, f"{name}_dout": dout, f"{name}_out64": o64, f"{name}_dx64": ref["x"], f"{name}_nbt": np.int64(nbt)})
        for k in TR.PARAMS:
            rec[f"{name}_d{k}64"] = ref[k]
        for k in TR.RUNNING:
            rec[f"{name}_{k}64"] = np.asarray(r64[k], np.float64)
        yard = TR.distances(got, ref, training)
        for q in TR.QUANTITIES:
            rec[f"{name}_yard_{q}"] = np.float64(yard[q])
        print(f"{name}: restatement fp64 {max(dm.values()):.2e}; yardsticks " + " ".join(f"{q} {yard[q]:.3g}" for q in TR.QUANTITIES))
    rec["classes_bit_identical"] = np.bool_(identical)
    np.savez_compressed(TR.GOLDEN, **rec)
    print("wrote", TR.GOLDEN, os.path.getsize(TR.GOLDEN), "bytes;", len(rec), "keys")
    if "--tolerance" in sys.argv:
        write_tolerance(np.load(TR.GOLDEN, allow_pickle=False))


def record_kernel_figures(log):
    """{case: {quantity: figure}} from the lines `golden <case>: out .. dparams .. dx .. running ..` and `<edge key>: ...` of a test log."""
    import re
    worst = {}
    for line in open(log):
        m = re.match(r"^\.*(?:golden )?([a-z0-9x]+(?:-train|-eval)?): (out [0-9.e+-]+ dparams .*)$", line.strip())
        if m and "against the record" not in line:
            f = m.group(2).split()
            worst[m.group(1)] = {f[i]: float(f[i + 1]) for i in range(0, 8, 2)}
    with open(TR.TOLERANCE) as fh:
        doc = json.load(fh)
    doc["kernel_worst"] = worst
    with open(TR.TOLERANCE, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("recorded the kernels' figures of", len(worst), "cases")


def write_tolerance(z):
    old = {}
    if os.path.exists(TR.TOLERANCE):
        with open(TR.TOLERANCE) as f:
            old = json.load(f)
    per_case = TR.floors(z)
    floors = {q: max(r[q] for r in per_case.values()) for q in TR.QUANTITIES}
    cases_ = []
    for name, r in per_case.items():
        row = {"case": name, "shape_BGnC": list(SHAPE) + [C]}
        for q in TR.QUANTITIES:
            row[f"{q}_yardstick"], row[f"{q}_restatement_f32"] = float(z[f"{name}_yard_{q}"]), r[q]
        cases_.append(row)
    edges = {}
    for shape, training in TR.EDGE_MODES:
        fl = TR.edge_floor(shape, training)
        edges[TR.edge_key(shape, training)] = {"floors": fl, "bars": {q: 2.0 * max(fl[q], floors[q]) for q in TR.QUANTITIES}}
        print(TR.edge_key(shape, training), fl, flush=True)
    doc = {"unit": "max|x - reference fp64| / max|reference fp64| for out, the worst parameter gradient, d(point_groups) and the worst "
                   "running statistic; db1, db2 and db3 in training mode on the scale of max|dbeta| of the BatchNorm they feed",
           "rule": "bar = 2 x floor per quantity.  floor: the largest distance of the fp32 restatement in the kernels' order "
                   "(tests/tokenizer_ref.py) from the fp64 record over the golden cases, measured on the CPU; gradients are compared under "
                   "the compared side's own max decisions (arg2 / arg4), which are checked separately.  The yardsticks (the reference's own "
                   "fp32 run against its fp64 run) are recorded and set no bar.",
           "floors": floors, "bars": {q: 2.0 * v for q, v in floors.items()}, "cases": cases_,
           "edge_rule": "A shape without a recorded case has a floor of its own, measured the same way on the CPU on the test's own "
                        "(seeded) inputs: the fp32 restatement in the kernels' order against the fp64 restatement.  bar = 2 x max(floor of "
                        "the golden cases, floor of the shape).  The reason: BatchNorm over few points is ill-conditioned (with two points "
                        "x-hat is +-1 whatever the input and every input gradient is a difference of nearly equal numbers), so what fp32 "
                        "can hold there is up to twenty times coarser than at the golden cases; and db1, db2, db3, sums of rounding errors "
                        "held on dbeta's scale, grow with the rows.  At every shape the gradients are compared under the compared side's "
                        "own max AND ReLU decisions: both are discontinuous, and among the 8 million ReLU decisions of the workload-shaped "
                        "case some pre-activation always lies within rounding of zero.",
           "edge_cases": edges,
           "kernel_worst": old.get("kernel_worst"),
           "kernel_worst_source": "tests/test_gpu_tokenizer.py::test_golden_cases and ::test_edge_shapes on one MI355X (the figures they "
                                  "print), same unit"}
    os.makedirs(os.path.dirname(TR.TOLERANCE), exist_ok=True)
    with open(TR.TOLERANCE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", TR.TOLERANCE, floors)


if __name__ == "__main__":
    if "--kernel-log" in sys.argv:
        record_kernel_figures(sys.argv[sys.argv.index("--kernel-log") + 1])
    else:
        main()

"""SHA-256 of the output buffers of the five loss entry points (csrc/loss.hip) on fixed inputs: the bit-identity record of a refactor.

    python tools/loss_digest.py                                   print the digests of the current build
    python tools/loss_digest.py --record FILE --commit HASH --hipcc "LINE"
                                                                  write them as tests/golden/loss_bits.json holds them

`digests(gpu)` is the one place that builds the inputs, makes the calls and hashes the raw bytes of probs, loss_rows, kd_rows and
dlogits; tests/test_loss_bits_gpu.py calls it and compares with the recorded file.  X3D_HIP_LIB selects the library (hip.py), so a
record is taken with the library of the commit it names.

Shapes   N in {1, 3} x M in {1, 157, 256, 257, 400}: one class, under one 256-thread round, exactly one, one element into the
         second, the product's size.
Rows     three kinds.  N = 3 has one of each, N = 1 takes kind (index of M) mod 3:
           0  ordinary logits; a multi-hot target row for the sigmoid head
           1  one logit 40 above the rest (p < 1e-7 and p > 1 - 1e-7 both occur; the label is that class when the index of M is
              even, a random one when it is odd); soft multi-label targets; a non-finite teacher logit (+inf when the index of M
              is even, NaN when it is odd)
           2  a label outside [0, M) (M or -1) and a NaN in the dense target row; the teacher is finite
Calls    every entry point with loss and gradient both, loss_rows (and kd_rows) null, dlogits null; the three plain entry points
         also probs only.  One digest per (entry point, shape, outputs, alpha) over the calls with grad_scale in {1, 1/64} and, for
         the distillation forms, T in {1, 4}, in that order.  Null outputs aside, every output buffer is filled with 123 before the
         call and hashed whole after it, so a store that goes missing shows as much as one that changes."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NS = (1, 3)
MS = (1, 157, 256, 257, 400)
GRAD_SCALES = (1.0, 1.0 / 64.0)
ALPHAS = (0.0, 0.5, 1.0)
TEMPERATURES = (1.0, 4.0)
OUTPUTS = ("both", "no_loss", "no_grad")


def _inputs(n, m, mi):
    """host arrays of one shape: logits, teacher, labels, dense softmax targets, multi-label targets"""
    rng = np.random.RandomState(1000 * n + m)
    kinds = [0, 1, 2] if n == 3 else [mi % 3]
    z = (3.0 * rng.randn(n, m)).astype(np.float32)
    t = (3.0 * rng.randn(n, m)).astype(np.float32)
    labels = rng.randint(0, m, size=n).astype(np.int32)
    a, b = rng.randint(0, m, size=n), rng.randint(0, m, size=n)
    lam = rng.rand(n).astype(np.float32)
    soft = np.full((n, m), np.float32(0.1) / np.float32(m), dtype=np.float32)
    multi = (rng.rand(n, m) < 0.1).astype(np.float32)
    for r, kind in enumerate(kinds):
        soft[r, a[r]] += np.float32(0.9) * lam[r]
        soft[r, b[r]] += np.float32(0.9) * (np.float32(1.0) - lam[r])
        if kind == 1:
            z[r, m // 2] += np.float32(40.0)
            if mi % 2 == 0:
                labels[r] = m // 2                           # the label is the class above the range
            multi[r] = rng.rand(m).astype(np.float32)
            t[r, m // 3] = np.inf if mi % 2 == 0 else np.nan
        if kind == 2:
            labels[r] = m if mi % 2 == 0 else -1
            soft[r, (2 * m) // 3] = np.nan
            multi[r, (2 * m) // 3] = np.nan
    return z, t, labels, soft, multi


def _sha_calls(gpu, n, m, outputs, kd, calls):
    """one digest over `calls`: each a function of (probs, loss_rows, kd_rows, dlogits) that makes one launch"""
    h = hashlib.sha256()
    for call in calls:
        fill = lambda *shape: torch.full(shape, 123.0, dtype=torch.float32, device=gpu)
        probs = fill(n, m)
        loss_rows = fill(n) if outputs in ("both", "no_grad") else None
        kd_rows = fill(n) if kd and outputs in ("both", "no_grad") else None
        dlogits = fill(n, m) if outputs in ("both", "no_loss") else None
        call(probs, loss_rows, kd_rows, dlogits)
        for name, buf in (("probs", probs), ("loss_rows", loss_rows), ("kd_rows", kd_rows), ("dlogits", dlogits)):
            if buf is not None:
                a = np.ascontiguousarray(buf.cpu().numpy())
                h.update(name.encode() + b"\0")
                h.update(memoryview(a.view(np.uint8).reshape(-1)))
    return h.hexdigest()


def digests(gpu):
    """{entry: sha256 hex} in a fixed order (insertion order of the dict)"""
    from x3d_tf_amd import ops
    out = {}
    for n in NS:
        for mi, m in enumerate(MS):
            z, t, labels, soft, multi = (torch.from_numpy(a).to(gpu) for a in _inputs(n, m, mi))
            shape = f"N{n}M{m}"
            plain = (("softmax_xent", ops.softmax_xent, labels), ("softmax_xent_soft", ops.softmax_xent_soft, soft),
                     ("sigmoid_bce", ops.sigmoid_bce, multi))
            for name, fn, tgt in plain:
                out[f"{name}/{shape}/probs_only"] = _sha_calls(
                    gpu, n, m, "probs_only", False, [lambda p, l, k, d, fn=fn: fn(z, None, p)])
                for outputs in OUTPUTS:
                    out[f"{name}/{shape}/{outputs}"] = _sha_calls(
                        gpu, n, m, outputs, False,
                        [lambda p, l, k, d, fn=fn, tgt=tgt, gs=gs: fn(z, tgt, p, l, d, gs) for gs in GRAD_SCALES])
            kd = (("softmax_xent_kd/labels", lambda p, l, k, d, **kw: ops.softmax_xent_kd(z, t, p, labels=labels, loss_rows=l, kd_rows=k, dlogits=d, **kw)),
                  ("softmax_xent_kd/targets", lambda p, l, k, d, **kw: ops.softmax_xent_kd(z, t, p, targets=soft, loss_rows=l, kd_rows=k, dlogits=d, **kw)),
                  ("sigmoid_bce_kd", lambda p, l, k, d, **kw: ops.sigmoid_bce_kd(z, t, multi, p, loss_rows=l, kd_rows=k, dlogits=d, **kw)))
            for name, fn in kd:
                for outputs in OUTPUTS:
                    for alpha in ALPHAS:
                        out[f"{name}/{shape}/{outputs}/alpha{alpha}"] = _sha_calls(
                            gpu, n, m, outputs, True,
                            [lambda p, l, k, d, fn=fn, gs=gs, T=T, alpha=alpha: fn(p, l, k, d, grad_scale=gs, alpha=alpha, temperature=T)
                             for gs in GRAD_SCALES for T in TEMPERATURES])
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", metavar="FILE", help="write the fixture here instead of printing the digests")
    ap.add_argument("--commit", help="the commit the library in use was built from (--record)")
    ap.add_argument("--hipcc", help="the `hipcc --version` line of the compiler it was built with (--record)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_digest.py runs the kernels: it needs the GPU"
    d = digests(torch.device("cuda:0"))
    if not args.record:
        for k, v in d.items():
            print(v, k)
        return
    assert args.commit and args.hipcc, "--record needs --commit and --hipcc: the digests belong to that source and compiler"
    with open(args.record, "w") as fh:
        json.dump(dict(commit=args.commit, hipcc=args.hipcc, device=torch.cuda.get_device_name(0), digests=d), fh, indent=1)
        fh.write("\n")
    print(f"{len(d)} digests -> {args.record}")


if __name__ == "__main__":
    main()

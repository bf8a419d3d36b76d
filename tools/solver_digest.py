"""SHA-256 of every output buffer of every entry point of csrc/solver.hip on fixed inputs: the bit-identity record of a refactor.

    python tools/solver_digest.py                                   print the digests of the current build
    python tools/solver_digest.py --record FILE --commit HASH --hipcc "LINE"
                                                                    write them as tests/golden/solver_bits.json holds them

`digests(gpu)` is the one place that builds the inputs, makes the calls and hashes the raw bytes of w, the slots, ema, acc, out,
partials[:used] and q; tests/test_solver_bits_gpu.py calls it and compares with the recorded file.  X3D_HIP_LIB selects the library
(hip.py), so a record is taken with the library of the commit it names.

Inputs: the builders the solver tests use (tests/solver_cases.py).
  flat kernels    CASES of tests/test_solver_gpu.py (n = 1 ... 4100, 2 500 003 for the second grid sweep, every pointer one float
                  off, no mask), each with extras in {none, a norm that clips, a norm that does not, ema, norm + ema}; a
                  non-finite gradient once.
  chunk kernels   the _fix layout of tests/test_layerwise_gpu.py (NaN padding), aligned and one float off, the same extras, LARS
                  clip on and off, LAMB decay 0 and 0.01; a non-finite gradient once.
max_norm comes from the device's own sum of squares (math.sqrt of out[0]) and not from a host sum, whose order is numpy's to choose
(_fix's norm_total is such a sum; nothing here reads it)."""
import argparse
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTRAS = ["none", "clip", "noclip", "ema", "clip_ema"]
DECAY = float(np.float32(0.9))


def _sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(memoryview(a.view(np.uint8).reshape(-1))).hexdigest()


def _max_norm(norm, gs, mode):
    """half the unscaled global norm (clips) or twice it plus one (does not), from the device's fp64 sum of squares"""
    total = math.sqrt(float(norm[0].item())) * float(gs)
    return 0.5 * total if mode.startswith("clip") else 2.0 * total + 1.0


def _flat(gpu, out):
    from tests import solver_cases as T
    from x3d_tf_amd import hip, ops
    gs = float(np.float32(1.0 / 1024.0))
    for (n, off, with_mask), cid in zip(T.CASES, T.IDS):
        w, v, g, mask = T._host(n, 21)
        mask = mask if with_mask else None
        m2 = (np.abs(v) * 0.01).astype(np.float32)
        e = (0.5 * w + 0.1).astype(np.float32)
        dev = lambda *arrays: [T._dev(a, gpu, off) for a in arrays]
        put = lambda key, names, tensors: out.update({f"flat/{cid}/{key}/{k}": _sha(t) for k, t in zip(names, tensors)})
        gd, = dev(g)
        scratch = torch.zeros(int(hip.load().x3d_grad_sumsq_scratch(n)), dtype=torch.float64, device=gpu)
        norm = ops.grad_sumsq(gd, scratch=scratch)
        put("grad_sumsq", ("out", "scratch"), (norm, scratch))
        a = dev(w, v, g, mask)
        T._sgd_plain(*a, gs)
        put("sgd", "wv", a)
        a = dev(w, v, m2, g, mask)
        T._adam_plain(*a, gs)
        put("adam", "wmv", a)
        for mode in EXTRAS:
            kw = {}
            if mode != "none" and mode != "ema":
                kw.update(norm=norm, max_norm=_max_norm(norm, gs, mode))
            if mode.endswith("ema"):
                kw.update(ema=dev(e)[0], decay=DECAY)
            a = dev(w, v, g, mask)
            T._sgd_ex(*a, gs, **kw)
            put(f"sgd_ex/{mode}", "wve", a[:2] + [kw["ema"]] if "ema" in kw else a[:2])
            if "ema" in kw:
                kw["ema"] = dev(e)[0]
            a = dev(w, v, m2, g, mask)
            T._adam_ex(*a, gs, **kw)
            put(f"adam_ex/{mode}", "wmve", a[:3] + [kw["ema"]] if "ema" in kw else a[:3])
        ed, wd_ = dev(e, w)
        ops.ema_update(ed, wd_, DECAY)
        put("ema_update", ("ema",), (ed,))
        ops.ema_update(ed, wd_, DECAY, norm)
        put("ema_update/norm", ("ema",), (ed,))
        acc, = dev(w)
        ops.grad_accum(acc, gd, first=True)
        put("grad_accum/first", ("acc",), (acc,))
        acc, = dev(w)
        ops.grad_accum(acc, gd)
        put("grad_accum/add", ("acc",), (acc,))
        if cid == "n4100":                                   # (once: aliasing, and the non-finite gradient)
            g2, = dev(g)
            ops.grad_accum(g2, g2)
            put("grad_accum/alias", ("acc",), (g2,))
            gbad = g.copy()
            gbad[n // 2] = np.inf
            gb, = dev(gbad)
            nb = ops.grad_sumsq(gb)
            wd_, vd, md, ed, kd = dev(w, v, m2, e, mask)
            T._sgd_ex(wd_, vd, gb, kd, 1.0, nb, 1.0, ed, DECAY)
            T._adam_ex(wd_, vd, md, gb, kd, 1.0, nb, 1.0, ed, DECAY)
            ops.ema_update(ed, wd_, DECAY, nb)
            put("nonfinite", ("out", "w", "v", "m", "ema"), (nb, wd_, vd, md, ed))


def _chunks(gpu, out):
    from tests import solver_cases as T
    from x3d_tf_amd import ops
    f = T._fix(gpu)
    gs = float(T.GS)
    nseg = len(T.LENGTHS)
    for off in (0, 1):
        masters = {k: T._dirty(f, a, gpu, off)[0] for k, a in dict(w=f.w, v=f.v, v2=f.v2, g=f.g, e=f.e).items()}

        def fresh(*keys):
            """copies of the NaN-padded device arrays at the same alignment"""
            res = []
            for k in keys:
                buf = torch.empty(f.n + off + 8, dtype=torch.float32, device=gpu)
                res.append(buf[off:off + f.n].copy_(masters[k]))
            return res

        def scratch():
            return (torch.zeros(2 * f.table.nchunk, dtype=torch.float64, device=gpu),
                    torch.ones(nseg, dtype=torch.float32, device=gpu))

        tag = "chunks/off%d" % off
        put = lambda key, names, tensors: out.update({f"{tag}/{key}/{k}": _sha(t) for k, t in zip(names, tensors)})
        gd = masters["g"]
        part = torch.zeros(f.table.nchunk, dtype=torch.float64, device=gpu)
        put("seg_sumsq", ("out", "partials"), (ops.seg_sumsq(gd, f.table, partials=part), part))
        norm = T._norm_of(f.g, gpu)

        def run_all(key, kw, ema_of):
            for clip in (False, True):
                (wd_, vd), (p, q), ed = fresh("w", "v"), scratch(), ema_of()
                h = T.LARS
                ops.lars(wd_, vd, gd, f.table, h["lr"], h["mom"], h["wd"], h["eta"], h["eps"], clip, partials=p, q=q,
                         **dict(kw, ema=ed))
                put(f"lars{'_clip' if clip else ''}/{key}", ("w", "v", "partials", "q", "ema"), [wd_, vd, p, q] + ([ed] if ed is not None else []))
            (wd_, md, vd), ed = fresh("w", "v", "v2"), ema_of()
            h = T.SEG_ADAM
            ops.adamw(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], np.float32(0.05), **dict(kw, ema=ed))
            put(f"adamw/{key}", "wmve", [wd_, md, vd] + ([ed] if ed is not None else []))
            for decay in (0.0, 0.01):
                (wd_, md, vd), (p, q), ed = fresh("w", "v", "v2"), scratch(), ema_of()
                h = T.LAMB
                ops.lamb(wd_, md, vd, gd, f.table, h["lr"], h["step"], h["b1"], h["b2"], h["eps"], decay, partials=p, q=q,
                         **dict(kw, ema=ed))
                put(f"lamb_decay{decay}/{key}", ("w", "m", "v", "partials", "q", "ema"), [wd_, md, vd, p, q] + ([ed] if ed is not None else []))

        for mode in EXTRAS:
            kw = dict(grad_scale=gs)
            if mode != "none" and mode != "ema":
                kw.update(norm=norm, max_norm=_max_norm(norm, gs, mode))
            if mode.endswith("ema"):
                kw.update(ema_decay=DECAY)
            run_all(mode, kw, (lambda: fresh("e")[0]) if mode.endswith("ema") else (lambda: None))
        if off == 0:                                         # (once: a non-finite gradient skips every launch)
            g = f.g.copy()
            g[f.segs[5][0] + 7] = np.inf
            nb = T._norm_of(g, gpu)
            gd = T._dirty(f, g, gpu)[0]
            run_all("nonfinite", dict(grad_scale=gs, norm=nb, max_norm=1.0, ema_decay=DECAY), lambda: fresh("e")[0])


def digests(gpu):
    """{entry: sha256 hex} in a fixed order (insertion order of the dict)"""
    out = {}
    _flat(gpu, out)
    _chunks(gpu, out)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", metavar="FILE", help="write the fixture here instead of printing the digests")
    ap.add_argument("--commit", help="the commit the library in use was built from (--record)")
    ap.add_argument("--hipcc", help="the `hipcc --version` line of the compiler it was built with (--record)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "solver_digest.py runs the kernels: it needs the GPU"
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

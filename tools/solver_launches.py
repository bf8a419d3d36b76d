"""Every solver launch of a Trainer.step, name and argument tuple, for a grid of configurations: the launch-for-launch record of
a refactor of the Python side of the optimizer update.

    python tools/solver_launches.py                          print the launches of the current tree
    python tools/solver_launches.py --record FILE --commit HASH
                                                             write them as tests/golden/solver_launches.json holds them

`launches(gpu)` is the one place that builds the trainers, spies on `hip.call` and writes the calls down;
tests/test_solver_launches_gpu.py calls it and compares with the recorded file.  Only the public Trainer / X3D API is used, so the
tool runs unchanged on either side of such a refactor.

What is recorded, per case and per Trainer.step (two steps each: the first allocates what is allocated lazily, the second of the
ACCUM_STEPS = 2 case is the one that updates): the calls whose name belongs to the solver family, in order, as [name, [args]].
  scalars    by repr (the Python value handed to ctypes: 0.1 and 0.1f are told apart by the entry point, not here)
  pointers   flat_params, flat_velocity, flat_second, flat_grads, l2_mask and ema by name, "+k" for an element offset into them;
             every other pointer p0, p1, ... in order of first appearance within the step; null as None
Which arguments are pointers is read from the loaded library's argtypes (include/x3d_hip.h).

Cases: the five rules x {no extras, SOLVER.CLIP_GRAD_L2NORM, clip + SOLVER.EMA_DECAY} x {plain, SOLVER.FREEZE + LAYER_DECAY};
float16 storage with dynamic loss scaling (the finite check), flat and fine-tuned; ACCUM_STEPS = 2.  X3D-XS, 10 classes, no
dropout, 2 clips of 4 x 32 x 32: the arguments do not depend on the workload's size."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RULES = ("sgd", "adam", "lars", "adamw", "lamb")
EXACT = ("x3d_grad_sumsq", "x3d_seg_grad_sumsq", "x3d_all_finite", "x3d_sgd_pt", "x3d_ema_update", "x3d_grad_accum")
PREFIXES = ("x3d_sgd_nesterov", "x3d_adam", "x3d_lars", "x3d_lamb")
OPTS = ["DATA.TEMP_DURATION", 4, "DATA.TRAIN_CROP_SIZE", 32, "DATA.TEST_CROP_SIZE", 32, "TEST.NUM_TEMPORAL_VIEWS", 1,
        "TEST.NUM_SPATIAL_CROPS", 3, "TEST.BATCH_SIZE", 2, "NETWORK.NUM_CLASSES", 10, "NETWORK.DROPOUT_RATE", 0.0,
        "TRAIN.BATCH_SIZE", 2, "TRAIN.DATASET_SIZE", 4, "TRAIN.EPOCHS", 2, "OPTIM.LARS_TRUST_COEF", 0.02, "OPTIM.WEIGHT_DECAY", 0.01]
EXTRAS = dict(none=[], clip=["SOLVER.CLIP_GRAD_L2NORM", 0.05], clip_ema=["SOLVER.CLIP_GRAD_L2NORM", 0.05, "SOLVER.EMA_DECAY", 0.5])
FINETUNE = dict(plain=[], ft=["SOLVER.FREEZE", ["conv1/", "stages/0/", "stages/1/"], "SOLVER.LAYER_DECAY", 0.9])
STEPS, LR = 2, 0.05


def cases():
    """{case name: (config options, storage type)}"""
    out = {}
    for rule in RULES:
        for ex, ex_opts in EXTRAS.items():
            for ft, ft_opts in FINETUNE.items():
                out[f"{rule}/{ex}/{ft}"] = (["TRAIN.OPTIMIZER", rule] + ex_opts + ft_opts, torch.float32)
    out["fp16/sgd/none/plain"] = (["TRAIN.OPTIMIZER", "sgd"], torch.float16)
    out["fp16/adamw/clip/ft"] = (["TRAIN.OPTIMIZER", "adamw"] + EXTRAS["clip"] + FINETUNE["ft"], torch.float16)
    out["accum2/sgd/clip_ema/plain"] = (["TRAIN.OPTIMIZER", "sgd", "SOLVER.ACCUM_STEPS", 2] + EXTRAS["clip_ema"], torch.float32)
    return out


def _is_solver(name):
    return name in EXACT or name.startswith(PREFIXES)


class _Names:
    """pointer -> symbol, for one step"""

    def __init__(self, model, trainer):
        self.model, self.trainer, self.other = model, trainer, {}

    def __call__(self, p):
        if p is None:
            return None
        named = [(k, getattr(self.model, k, None)) for k in ("flat_params", "flat_velocity", "flat_second", "flat_grads", "l2_mask")]
        named.append(("ema", self.trainer.ema))
        for k, t in named:
            if t is not None and t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
                off = (p - t.data_ptr()) // t.element_size()
                return k if off == 0 else f"{k}+{off}"
        return self.other.setdefault(p, f"p{len(self.other)}")


def _one_case(opts, dtype, gpu, batches):
    import x3d_tf_amd as x
    from x3d_tf_amd import hip
    from x3d_tf_amd.model import X3D
    from x3d_tf_amd.train import Trainer
    cfg = x.get_config("XS", OPTS + opts)
    m = X3D(cfg, dtype=dtype, device=gpu, seed=1)
    tr = Trainer(m, cfg)
    lib, real, steps = hip.load(), hip.call, []

    def spy(name, *args):
        if _is_solver(name):
            kinds = getattr(lib, name).argtypes[:-1]          # (the last one is the stream hip.call appends)
            assert len(kinds) == len(args), (name, len(kinds), len(args))
            steps[-1].append([name, [names(a) if k is ctypes.c_void_p else repr(a) for k, a in zip(kinds, args)]])
        return real(name, *args)

    hip.call = spy
    try:
        for clips, labels in batches:
            names = _Names(m, tr)
            steps.append([])
            tr.step(clips, labels, LR)
    finally:
        hip.call = real
    torch.cuda.synchronize()
    return steps


def launches(gpu):
    """{case: [the solver calls of step 1, of step 2]}, each call [name, [args]]"""
    gen = torch.Generator().manual_seed(5)
    batches = [(torch.randn(2, 4, 32, 32, 3, generator=gen).to(gpu), torch.randint(0, 10, (2,), generator=gen).to(gpu))
               for _ in range(STEPS)]
    return {name: _one_case(opts, dtype, gpu, batches) for name, (opts, dtype) in cases().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", metavar="FILE", help="write the fixture here instead of printing the launches")
    ap.add_argument("--commit", help="the commit of the tree in use (--record)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "solver_launches.py makes the launches: it needs the GPU"
    d = launches(torch.device("cuda:0"))
    if not args.record:
        for case, steps in d.items():
            for i, calls in enumerate(steps):
                for name, a in calls:
                    print(f"{case} step {i + 1}: {name}({', '.join(map(str, a))})")
        return
    assert args.commit, "--record needs --commit: the launches belong to that tree"
    with open(args.record, "w") as fh:              # one call per line: a difference reads as a one-line diff
        fh.write('{"commit": %s, "device": %s, "cases": {\n' % (json.dumps(args.commit), json.dumps(torch.cuda.get_device_name(0))))
        fh.write(",\n".join(' %s: [\n%s\n ]' % (json.dumps(case), ",\n".join(
            "  [\n%s\n  ]" % ",\n".join("   " + json.dumps(call) for call in calls) for calls in steps)) for case, steps in d.items()))
        fh.write("\n}}\n")
    print(f"{sum(len(c) for s in d.values() for c in s)} launches of {len(d)} cases -> {args.record}")


if __name__ == "__main__":
    main()

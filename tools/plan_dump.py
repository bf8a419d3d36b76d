"""Canonical text dump of a DRY plan's launch lists, for comparing two source trees launch for launch.

    python tools/plan_dump.py TREE (--config K | --shape VARIANT N T S DTYPE train|infer) [--opt NAME=0|1 ...] [--cfg KEY VALUE ...]

imports the package from TREE (so one copy of this script serves both trees), records the plan on a dry model and prints one
line per entry of pl.fwd then pl.bwd -- entry name, every positional argument, the argument struct field by field (nested
structs, arrays of structs, pointer-to-struct fields and host structs referred to by address followed) -- then the decoded
bn_eval_table, bwd_stage_marks, input_slots and the bytes the plan allocated.  A dry device buffer prints as its offset from
the first dry address of the process (d+0x...), any other address as a label numbered by first appearance (h0, h1, ...).
Two trees record the same plan exactly when their dumps are byte-identical (`cmp`)."""
import argparse
import ctypes as C
import sys

ap = argparse.ArgumentParser()
ap.add_argument("tree")
ap.add_argument("--config", type=int)
ap.add_argument("--shape", nargs=6, metavar=("VARIANT", "N", "T", "S", "DTYPE", "MODE"))
ap.add_argument("--opt", action="append", default=[], help="plan option, NAME=0|1")
ap.add_argument("--cfg", nargs=2, action="append", default=[], metavar=("KEY", "VALUE"))
args = ap.parse_args()
sys.path.insert(0, args.tree)
import torch  # noqa: E402
from x3d_tf_amd import hip, model as M  # noqa: E402
from x3d_tf_amd.config import get_config  # noqa: E402
from x3d_tf_amd.dispatch import BASELINE_CONFIGS  # noqa: E402

if args.config:
    variant, n, t, s, dtype, training, over = BASELINE_CONFIGS[args.config]
else:
    variant, n, t, s, dtype, training, over = (args.shape[0], int(args.shape[1]), int(args.shape[2]), int(args.shape[3]),
                                               getattr(torch, args.shape[4]), args.shape[5] == "train", {})
flat = [x for kv in list(over.items()) + [(k, eval(v)) for k, v in args.cfg] for x in kv]
base = M._FakeBuf._next
m = M.X3D(get_config(variant, flat or None), dtype=dtype, device="dry",
          options={k: bool(int(v)) for k, v in (o.split("=") for o in args.opt)})
pl = m._plan(n, t, s, s, training)
end = M._FakeBuf._next
labels = {}


def addr(v):
    if not v:
        return "0"
    return f"d+{v - base:#x}" if base <= v < end else labels.setdefault(v, f"h{len(labels)}")


def struct(st):
    out = [type(st).__name__]
    for f, ty in st._fields_:
        v = getattr(st, f)
        if ty is C.c_void_p:
            out.append(f"{f}={addr(v)}")
            if f == "coef_fold" and v in hip.FOLDS:      # a host struct referred to by address
                out.append("->" + struct(hip.FOLDS[v]))
        elif isinstance(v, C.Structure):
            out.append(f"{f}={struct(v)}")
        elif isinstance(v, C.Array):
            out.append(f"{f}=[" + ",".join(struct(i) if isinstance(i, C.Structure) else repr(i) for i in v) + "]")
        elif isinstance(v, C._Pointer):
            out.append(f"{f}=" + (struct(v.contents) if v else "0"))
        else:
            out.append(f"{f}={v!r}")
    return "(" + " ".join(out) + ")"


def value(x, ctype):
    if x is None or isinstance(x, (bool, float)):
        return repr(x)
    if isinstance(x, int):
        return addr(x) if ctype is C.c_void_p else str(x)
    if isinstance(x, C.Array):
        return "[" + ",".join(struct(j) for j in x) + "]"
    return "&" + struct(x._obj)      # C.byref(argument struct)


for tag, lst in (("fwd", pl.fwd), ("bwd", pl.bwd)):
    for i, (name, fn, a) in enumerate(lst):
        st = pl.structs.get((id(lst), i))
        byref = any(getattr(x, "_obj", None) is st for x in a)      # (the struct the plan remembers is normally an argument)
        print(tag, i, name, *[value(x, ty) for x, ty in zip(a, fn.argtypes)], *([] if st is None or byref else ["struct=" + struct(st)]))
if getattr(pl, "bn_eval_table", None) is not None:
    raw = bytes(pl.bn_eval_table.cpu().numpy().tobytes())
    for k in range(len(raw) // C.sizeof(hip.BnEvalItem)):
        print("bn_eval", k, struct(hip.BnEvalItem.from_buffer_copy(raw, k * C.sizeof(hip.BnEvalItem))))
print("bwd_stage_marks", sorted(pl.bwd_stage_marks.items()))
print("input_slots", [("fwd" if lst is pl.fwd else "bwd" if lst is pl.bwd else "?", i, pos[0] if pos else 0)
                      for lst, i, *pos in pl.input_slots])
print("allocated", end - base, "device bytes,", pl.zero_buf.numel(), "fp64 accumulators")

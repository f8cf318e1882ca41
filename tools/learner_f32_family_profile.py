"""Writes learner_f32_family.txt into --out (default: profiles/ of this tree): for every case of tests/learner_f32_family.py that is held
to the float64 bars, per parameter block, the floor (the largest |f32 random-order variant - float64 model| over 8 seeds), the oracle's
error and the device's error against the float64 model — for the gradient of the last step and for the weights after the case's steps —
and the same for the losses; plus the number of entries in which the device's bits differ from the oracle's. Needs an MI355X; --no-gpu
writes the floors and the oracle's errors alone."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import learner_f32_family as lf  # noqa: E402
from tests import oracle_lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--no-gpu", action="store_true")
args = ap.parse_args()
orc = oracle_lib.load()
engines = {}
if not args.no_gpu:
    import synthesis_amd as sa

    for net in lf.NETS:
        engines[net] = sa.Engine(concurrent_games=64, max_explores=64)
        (engines[net].load_weights if net == "mlp" else engines[net].load_weights_conv)(lf.family(net)["init"])

lines = ["The f32 learners on the stress family of tests/learner_f32_family.py (tools/learner_f32_family_profile.py)"
         + ("" if args.no_gpu else ", device figures measured on an MI355X"),
         "case = network-member-variant-B-hyper-steps. Per block: floor / oracle error / device error (max |x - float64 model|), for the last",
         "step's gradient (g) and the weights after the steps (w); bar = 8 x floor. bits = entries (gradient, weights, m, v, losses) in which",
         "the device differs from the oracle. fragile = gate-fragile units of the first step (bars not asserted when > 0).", ""]
seen, total_bits = set(), 0
for c in lf.CASES:
    if c.route not in lf.BARRED_ROUTES or c.ref_key in seen:
        continue
    seen.add(c.ref_key)
    ref = lf.case_reference(c)
    orun = lf.final_state(lf.oracle_steps(orc, c.net, lf.family(c.net)[c.member], lf.case_batches(c), c.hyper, [lf.LR] * c.steps))
    oerr, olerr = lf.errors(c.net, ref, orun)
    derr = dlerr = None
    bits = "-"
    if engines:
        st, losses = lf.run_epoch(engines[c.net], c)   # one step or six through train_set_data + train_epoch
        drun = dict(st, losses=losses)
        derr, dlerr = lf.errors(c.net, ref, drun)
        nb = sum(int((np.asarray(drun[k], np.float32).view(np.uint32) != np.asarray(orun[k], np.float32).view(np.uint32)).sum())
                 for k in ("grads", "weights", "m", "v", "losses"))
        total_bits += nb
        bits = str(nb)
    fmt = lambda e: "-" if e is None else f"{e:.2e}"
    lines.append(f"{'-'.join(str(x) for x in c.ref_key)}  bits {bits}  fragile {ref['gate_fragile']}  losses floor {ref['loss_floor'].max():.2e} oracle "
                 f"{olerr.max():.2e} device {fmt(None if dlerr is None else dlerr.max())}")
    for name in lf.BLOCKS[c.net]:
        cells = []
        for k, tag in (("grads", "g"), ("weights", "w")):
            cells.append(f"{tag} {ref['floor'][k][name]:.2e} / {oerr[k][name]:.2e} / {fmt(None if derr is None else derr[k][name])}")
        lines.append(f"    {name:7s} " + "   ".join(cells))
lines.append("")
lines.append(f"{len(seen)} cases; entries in which the device's bits differ from the oracle's: {'-' if not engines else total_bits}")
for eng in engines.values():
    eng.close()
os.makedirs(args.out, exist_ok=True)
path = os.path.join(args.out, "learner_f32_family.txt")
with open(path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print("\n".join(lines[-3:]))
print("written", path, os.path.getsize(path), "bytes")

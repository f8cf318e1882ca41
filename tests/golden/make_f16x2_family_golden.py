"""Writes f16x2_family_device.npz and f16x2_checkpoint_family.txt into --out (default: tests/golden and profiles of this tree). Needs an
MI355X.

f16x2_family_device.npz: what the HIP engine's SYN_NET_ARITH_F16X2 arithmetic computes for 64 reachable positions under every member of
the stress family of tests/f16x2_checkpoints.py (both networks: raw logits, outcome probabilities, the plan the engine chose), committed
as tests/golden/f16x2_family_device.npz and replayed on the CPU by tests/test_oracle_f16x2.py / tests/test_conv_f16x2_model.py — the
restatements stay pinned to device-produced bits on the plan's caps, negative exponents and subnormal halves without a GPU.

f16x2_checkpoint_family.txt (committed as profiles/f16x2_checkpoint_family.txt): per member the plan's exponents, the outputs' scale and
the errors of the engine's f16x2 and f32 arithmetic against float64 on 1,000 positions, and the edges of the accepted whole-blob scalings.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import synthesis_amd as sa  # noqa: E402
from synthesis_amd.engine import f16x2_plan_of_blob  # noqa: E402
from tests import f16x2_checkpoints as fc  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests.test_gpu_parity import random_positions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="directory for both files (default: tests/golden and profiles)")
args = ap.parse_args()
npz_path = os.path.join(args.out or os.path.join(ROOT, "tests", "golden"), "f16x2_family_device.npz")
txt_path = os.path.join(args.out or os.path.join(ROOT, "profiles"), "f16x2_checkpoint_family.txt")
os.makedirs(os.path.dirname(npz_path), exist_ok=True)

orc = oracle_lib.load()
blob, trained, cblob, ctrained = fc.load_fixtures()
gmy, gop = random_positions(orc, 64, seed=4242)
gmy[0] = 0; gop[0] = 0
my, op = random_positions(orc, 1000, seed=2026)   # the positions of the CPU suite's f64 bars
out = dict(my_bb=gmy, op_bb=gop)
lines = ["f16x2 arithmetic on the stress family of tests/f16x2_checkpoints.py, measured on an MI355X (tests/golden/make_f16x2_family_golden.py)",
         "1,000 reachable positions; scale = max(1, max |raw_f64|); errors = max |logit - logit_f64| of the engine in either arithmetic;",
         "plan = activation exponents s / weight exponents t / out exponent (Connect4ConvNet: s = [0, s1], t = [tc, th])", ""]
eng = sa.Engine(concurrent_games=256, max_explores=16, device=0)
for net, fam, load, f64 in (("mlp", fc.mlp_family(blob, trained), eng.load_weights, fc.mlp_f64),
                            ("conv", fc.conv_family(cblob, ctrained), eng.load_weights_conv, fc.conv_f64)):
    lines.append({"mlp": "Connect4Net", "conv": "Connect4ConvNet"}[net])
    lines.append(f"{'member':24s} {'scale':>10s} {'f16x2 err':>10s} {'/scale':>9s} {'f32 err':>10s} {'value err':>10s}  plan")
    for name, w in fam.items():
        eng.set_network_arithmetic("f32")
        load(w)
        fl, _ = eng.policy_eval(my, op)
        eng.set_network_arithmetic("f16x2")
        _, plan = eng.network_arithmetic()
        l, v = eng.policy_eval(gmy, gop)
        out[f"{net}.{name}.logits"] = l; out[f"{net}.{name}.value"] = v
        out[f"{net}.{name}.plan"] = np.array(plan["activation_exp"] + plan["weight_exp"] + [plan["out_exp"]], np.int32)
        l, v = eng.policy_eval(my, op)
        f = fc.f64_errors(l, v, fl, *f64(w, my, op))
        nl = 5 if net == "mlp" else 2
        lines.append(f"{name:24s} {f['scale']:10.4g} {f['logit_err']:10.3e} {f['logit_err'] / f['scale']:9.2e} {f['f32_logit_err']:10.3e} "
                     f"{f['value_err']:10.3e}  s {plan['activation_exp'][:nl]} t {plan['weight_exp'][:nl]} out {plan['out_exp']}")
    _, e = fc.accept_edges(lambda x: f16x2_plan_of_blob(x) is not None, fam["init"])
    lines.append(f"init x 2^k, k = -30..30: accepted for k in [{e['last_accepted_down']}, {e['last_accepted_up']}], first refused below: "
                 f"{e['first_refused_down']}, above: {e['first_refused_up']}")
    lines.append("")
eng.close()
np.savez_compressed(npz_path, **out)
with open(txt_path, "w") as fh:
    fh.write("\n".join(lines))
print("\n".join(lines))
print("written", npz_path, os.path.getsize(npz_path), "bytes")

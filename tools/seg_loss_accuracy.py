#!/usr/bin/env python3
"""Relative errors of the fused and the composed segmentation loss against the fp64 restatement, per shape of
tests/_seg_loss_ref.py, as tests/test_gpu_seg_loss.py measures them.  Writes profiles/seg_loss_accuracy.json (or --out).

    python tools/seg_loss_accuracy.py [--out FILE]

Per shape: `grad` = relative L2 error of the gradient (fused, composed), `sums` = |d| / |ref| of every image's sum
(fused, composed).  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_loss_accuracy.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "seg_loss_accuracy needs a GPU"
    import _seg_loss_ref as R
    import test_gpu_seg_loss as T
    rows = []
    for i in range(len(R.SHAPES)):
        m = T.measure(i)
        rows.append({"shape_B_C_h_w_factor_H_W": m["shape"], "grad_rel_l2": {"fused": m["grad"][0], "composed": m["grad"][1]},
                     "sums_rel": [{"fused": f, "composed": c} for f, c in m["sums"]]})
    out = {"device": torch.cuda.get_device_name(0), "reference": "fp64 on the CPU (tests/_seg_loss_ref.py)", "shapes": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

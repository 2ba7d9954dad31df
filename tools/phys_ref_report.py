#!/usr/bin/env python3
"""Measure the fp64 physics reference's spreads and the deviations of the oracle and the HIP kernel.

    python tools/phys_ref_report.py --store     # (re)write tests/golden/phys_ref_spreads.npz, CPU only
    python tools/phys_ref_report.py --store --only plane,self   # re-measure these families, keep the rest
    python tools/phys_ref_report.py             # the table of profiles/phys_ref/README.md on stdout

Per family and robot: the median and the largest spread (phys_ref.sensitivity, k = 32) of the joint
velocities, the root velocity and the contact forces; the largest deviation of the oracle (CPU) and,
when a GPU is present, of the HIP kernel from the reference in the same quantities; the largest
deviation / spread over all quantity groups (the margin each would need) and the excluded cases.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("unitree-rl-gym_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import bridge  # noqa: E402
import phys_ref as pr  # noqa: E402
import test_phys_ref_host as H  # noqa: E402


def worst(fam, refs, spreads, got):
    dev = {g: 0.0 for g in pr.GROUPS}
    need = 0.0
    for e in range(fam.n):
        if refs[e]["excluded"]:
            continue
        d = pr.deviation(refs[e], dict(root=got["root"][e], q=got["q"][e], qd=got["qd"][e], cforce=got["cforce"][e]))
        for g in pr.GROUPS:
            dev[g] = max(dev[g], d[g])
            floor = 4 * pr.EPS32 * float(np.abs(refs[e][g]).max())
            if d[g] > floor and spreads[e][g] > 0:
                need = max(need, d[g] / spreads[e][g])
    return dev, need


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", action="store_true")
    ap.add_argument("--only", default="", help="with --store: comma-separated family names to re-measure; the rest is kept")
    args = ap.parse_args()
    lib = bridge.ensure_built()
    if args.store:
        only = set(filter(None, args.only.split(",")))
        out = dict(H.stored_spreads()) if only else {}
        for task, name in H.FAMILIES:
            if only and name not in only:
                continue
            fam = H.family(task, name)
            out[f"{task}/{name}"] = np.array([[pr.sensitivity(fam, e)[g] for g in pr.GROUPS] for e in range(fam.n)])
            print(task, name, fam.n, flush=True)
        np.savez_compressed(H.SPREADS, **out)
        return
    gpu = False
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        pass
    if gpu:
        from test_gpu_phys_reference import run_kernel
    print("| family | robot | N | excluded | spread qd med / max | spread v med / max | spread F/W med / max | "
          "oracle qd | oracle v | oracle F/W | oracle dev/spread | kernel qd | kernel v | kernel F/W | kernel dev/spread |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for task, name in H.FAMILIES:
        spec = H.spec_of(task)
        fam, refs, tols, spreads = H.reference(task, name)
        W = float(fam.model.mass.sum()) * 9.81
        col = lambda g, s=1.0: f"{np.median([x[g] for x in spreads]) / s:.1e} / {max(x[g] for x in spreads) / s:.1e}"  # noqa: E731
        odev, oneed = worst(fam, refs, spreads, H.run_oracle(lib, spec, fam, H.CHAIN[task]))
        cells = [name, task, fam.n, sum(r["excluded"] for r in refs), col("qd"), col("vlin"), col("cforce", W),
                 f"{odev['qd']:.1e}", f"{odev['vlin']:.1e}", f"{odev['cforce'] / W:.1e}", f"{oneed:.1f}"]
        if gpu:
            kdev, kneed = worst(fam, refs, spreads, run_kernel(spec, fam))
            cells += [f"{kdev['qd']:.1e}", f"{kdev['vlin']:.1e}", f"{kdev['cforce'] / W:.1e}", f"{kneed:.1f}"]
        else:
            cells += ["-"] * 4
        print("| " + " | ".join(str(c) for c in cells) + " |", flush=True)


if __name__ == "__main__":
    main()

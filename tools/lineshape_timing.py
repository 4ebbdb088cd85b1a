#!/usr/bin/env python3
"""HIP-event kernel time of one absorption model on the line-core pass of bench_voigt.py (50 000 lines, 400 000 grid points),
through mom_lineshape_xsec: `lineshape_timing.py SHAPE` with SHAPE one of voigt_sd, voigt15, doppler, lorentz prints one JSON line.
One shape per process, so that a caller can give every run its own time limit.  A measuring tool, not a test and not part of
bench.py."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench_voigt  # noqa: E402
import rtamd  # noqa: E402

SHAPES = {"voigt_sd": ("Voigt()", "HumlicekWeidemann32SDErrorFunction()"), "voigt15": ("Voigt()", "HumlicekWeidemann32VoigtErrorFunction()"),
          "doppler": ("Doppler()", "HumlicekWeidemann32SDErrorFunction()"), "lorentz": ("Lorentz()", "HumlicekWeidemann32SDErrorFunction()")}


def main(shape, repeats=5):
    model = rtamd.absorption.absorption_model(*SHAPES[shape])
    pf, grid, evals, _ = bench_voigt.workload()
    best = 1e30
    for _ in range(repeats):
        sig = rtamd._lib.lineshape_xsec(*model, pf.ν, pf.γ_d, pf.γ_l, pf.y, pf.S, pf.ind_start, pf.ind_stop, grid)
        best = min(best, rtamd._lib.voigt_last_kernel_ms())
    assert np.all(np.isfinite(sig)) and sig.min() >= 0 and sig.max() > 0
    print(json.dumps({"shape": shape, "kernel_ms": best, "evaluations": evals, "evaluations_per_s": evals / (best * 1e-3)}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "voigt_sd")

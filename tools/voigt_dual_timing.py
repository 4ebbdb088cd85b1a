#!/usr/bin/env python3
"""HIP-event kernel time of the value Voigt kernel and of its Dual run (sigma and its partials with respect to p and T) on
the workloads of bench_voigt.py: the line-core pass (same lines, same grid: k_voigt against k_voigt_dual) and the profile
operating point (two launches for all layers: mom_voigt_tau_abs_profile against mom_voigt_tau_abs_profile_dual).  Prints
one JSON line.  A measuring tool, not a test and not part of bench.py."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench_voigt  # noqa: E402
import rtamd  # noqa: E402


def main(repeats=5):
    ab = rtamd.absorption
    pf, grid, evals, core = bench_voigt.workload()
    tab = ab.synthetic_o2a_lines(50_000)
    pfd, dnu, dgd, dy, dS = ab.line_prefactors_dual(tab, grid, 150.0, 220.0, vmr=0.21, wing_cutoff=0.3)
    assert np.array_equal(pfd.ν, pf.ν) and np.array_equal(pfd.ind_start, pf.ind_start)
    val = dual = 1e30
    for _ in range(repeats):
        sig = rtamd.voigt_xsec(pf.ν, pf.γ_d, pf.y, pf.S, pf.ind_start, pf.ind_stop, grid)
        val = min(val, rtamd._lib.voigt_last_kernel_ms())
        sig_d, J = rtamd.voigt_xsec_dual(pf.ν, pf.γ_d, pf.y, pf.S, dnu, dgd, dy, dS, pf.ind_start, pf.ind_stop, grid)
        dual = min(dual, rtamd._lib.voigt_last_kernel_ms())
    assert np.max(np.abs(sig - sig_d)) <= 1e-13 * sig.max() and np.all(np.isfinite(J))
    out = {"line_core_pass": {"evaluations": evals, "weideman32_fraction": core / evals, "k_voigt_ms": val, "k_voigt_dual_ms": dual,
                              "ratio": dual / val}}
    tab, grid, p_full, T, vcd, evals, core = bench_voigt.profile_workload()
    m = rtamd.scenes.make_scene(1, 3, len(p_full), grid.size)
    val = dual = 1e30
    with rtamd.corert.make_handle(m) as h:
        for _ in range(repeats):
            val = min(val, ab.compute_absorption_profile(h, tab, grid, p_full, T, vcd, 0.21, wing_cutoff=40.0, model_vmr=0.21,
                                                         device_prefactors=True))
            dual = min(dual, ab.compute_absorption_profile(h, tab, grid, p_full, T, vcd, 0.21, wing_cutoff=40.0, model_vmr=0.21,
                                                           device_prefactors=True, dual=True))
    out["profile_operating_point"] = {"evaluations": evals, "weideman32_fraction": core / evals, "value_kernels_ms": val,
                                      "dual_kernels_ms": dual, "ratio": dual / val}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

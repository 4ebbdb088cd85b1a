#!/usr/bin/env python3
"""The phase-matrix Fourier moments (csrc/mom_zmom.hip, mom_z_moments) as a benchmark; prints one JSON line, `bench_zmoments.py
OUT.json` also writes it (committed as profiles/z_moments_bench.json).  `--host-repeats R` (default 3): runs of each host timing.

Three legs: the C2 shape (n = 3, the 20 nodes of scene_C2, Rayleigh + one set of l_max = 33, M = 3), the C4 shape (n = 4, 64 nodes,
Rayleigh + one set of l_max = 121, M = 3) and the C4 nodes with M = 32 and 1 + 4 sets of l_max = 121 (a value set and four
derivative sets).  Per leg: the HIP-event time of the two kernels, the wall time of compute_Z_moments_batch(device=0) and of the
host twin (device=None), both medians, and the contraction's share of the FP64 MFMA peak by its own operation count
2 * 2 * N^2 * n * sum over (set, m) of max(l_max - m, 0) over the event time (which includes the recurrence kernel).  For the C2
and C4 models also z_bases as the parent commit ran it (every (m, set) pair computed twice on the host) beside z_bases with
z_moments_on_device, in the same process on the same machine.

`--resident [OUT.json]` runs another leg instead and leaves the default output alone (committed as profiles/z_resident_bench.json):
for the C2 and C4 models the wall time from Greek coefficients to a set scene -- z_bases plus mom_scene_set, ended by a mom_sync,
median of 5, one handle, one process -- on three routes: Z on the host, Z by mom_z_moments and back through the host setter (the
round trip), and the staged Greek sets with the bases formed in the handle's memory (params.z_resident)."""
import dataclasses
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

PEAK_FP64_MFMA_TFLOPS = 78.6  # MI355X FP64 matrix spec


def _median_ms(f, repeats):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), t


def _parent_z_bases(rt, model):
    """z_bases of an unbanded model at the parent commit: two host calls per (m, Greek set)"""
    pol, μ = model.params.polarization_type, model.quad_points.qp_μ
    greeks = [model.greek_rayleigh] + [a.greek_coefs for a in model.aerosol_optics]
    Zpp = np.array([[rt.compute_Z_moments(pol, μ, g, m)[0] for g in greeks] for m in range(model.params.max_m)])
    Zmp = np.array([[rt.compute_Z_moments(pol, μ, g, m)[1] for g in greeks] for m in range(model.params.max_m)])
    return Zpp, Zmp


def run_leg(rtamd, pol, μ, greeks, M, host_repeats, device_repeats=5):
    rt, L = rtamd.corert, rtamd._lib
    n, N = pol.n, pol.n * μ.size
    rows = [(g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ) for g in greeks]
    ms = []
    for _ in range(device_repeats + 1):   # the first call loads the code objects
        Zd = L.z_moments(n, μ, rows, M)
        ms.append(Zd[2])
    gpu_ms = min(ms[1:])
    dev_ms, dev_all = _median_ms(lambda: rtamd.compute_Z_moments_batch(pol, μ, greeks, M, device=0), device_repeats)
    host = {}
    host_ms, host_all = _median_ms(lambda: host.update(Z=rtamd.compute_Z_moments_batch(pol, μ, greeks, M)), host_repeats)
    inner = sum(max(len(g.β) - m, 0) for g in greeks for m in range(M))
    flop = 2.0 * 2.0 * N * N * n * inner
    tf = flop / (gpu_ms * 1e-3) / 1e12
    Zdev = np.swapaxes(Zd[0], -1, -2)
    return {"nStokes": n, "n_mu": int(μ.size), "N": N, "sets": len(greeks), "l_max": [len(g.β) for g in greeks], "M": M,
            "kernels_ms": gpu_ms, "device_call_wall_ms": {"median": dev_ms, "runs": dev_all},
            "host_twin_wall_ms": {"median": host_ms, "runs": host_all}, "speedup_public_call": host_ms / dev_ms,
            "output_MB": 2 * 8.0 * N * N * len(greeks) * M / 1e6,
            "contraction": {"flop": flop, "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                                                       "frac": tf / PEAK_FP64_MFMA_TFLOPS}},
            "max_abs_device_minus_host": float(np.max(np.abs(Zdev - host["Z"][0]))), "max_abs_Z": float(np.max(np.abs(host["Z"][0])))}


def run_model(rtamd, model, host_repeats):
    rt = rtamd.corert
    md = dataclasses.replace(model, params=dataclasses.replace(model.params, z_moments_on_device=True))
    rt.z_bases(md)
    dev_ms, dev_all = _median_ms(lambda: rt.z_bases(md), 5)
    par_ms, par_all = _median_ms(lambda: _parent_z_bases(rt, model), host_repeats)
    now_ms, now_all = _median_ms(lambda: rt.z_bases(model), host_repeats)
    return {"z_bases_parent_host_route_ms": {"median": par_ms, "runs": par_all}, "z_bases_host_once_per_pair_ms": {"median": now_ms, "runs": now_all},
            "z_bases_on_device_ms": {"median": dev_ms, "runs": dev_all}, "speedup_vs_parent": par_ms / dev_ms,
            "device_faster_than_parent": bool(dev_ms < par_ms)}


def run_resident(repeats=5):
    import rtamd
    rt = rtamd.corert
    out = {"metric": "Greek coefficients to a set scene at the C4 shape (n = 4, 64 nodes, l_max = 121, M = 3): wall time of the resident route",
           "unit": "ms"}
    for name, m in (("C2", rtamd.scenes.scene_C2(S=8, Nz=2)), ("C4", rtamd.scenes.scene_C4(S=4, Nz=2))):
        sc = rt.prepare_scene(m)
        md = dataclasses.replace(m, params=dataclasses.replace(m.params, z_moments_on_device=True))

        def uploaded(h, model):
            Zpp, Zmp = rt.z_bases(model)
            rt.scene_set(h, dataclasses.replace(sc, Zpp=rt._abi_mats(Zpp), Zmp=rt._abi_mats(Zmp)))
            h.sync()

        def resident(h):
            rt.scene_set(h, dataclasses.replace(sc, Zpp=None, Zmp=None, greeks=rt.z_greeks(m)))
            h.sync()

        leg = {"N": sc.N, "K": sc.K, "M": sc.M, "Z_MB_each_way": 2 * 8.0 * sc.N * sc.N * sc.K * sc.M / 1e6}
        with rt.make_handle(m) as h:
            routes = (("host_z_ms", lambda: uploaded(h, m)), ("round_trip_device_z_ms", lambda: uploaded(h, md)), ("resident_ms", lambda: resident(h)))
            for key, f in routes:
                f()   # the first call loads the code objects
                med, runs = _median_ms(f, repeats)
                leg[key] = {"median": med, "runs": runs}
        leg["speedup_vs_round_trip"] = leg["round_trip_device_z_ms"]["median"] / leg["resident_ms"]["median"]
        leg["resident_faster_than_round_trip"] = bool(leg["resident_ms"]["median"] < leg["round_trip_device_z_ms"]["median"])
        out[name] = leg
    out["value"] = out["C4"]["resident_ms"]["median"]
    out["done"] = bool(out["C2"]["resident_faster_than_round_trip"] and out["C4"]["resident_faster_than_round_trip"])
    return out


def run(host_repeats=3):
    import rtamd
    rt = rtamd.corert
    c2, c4 = rtamd.scenes.scene_C2(S=8, Nz=2), rtamd.scenes.scene_C4(S=4, Nz=2)
    out = {"metric": "phase-matrix Fourier moments at the C4 shape (n = 4, 64 nodes, l_max = 121, M = 3): wall time of z_bases on the device",
           "unit": "ms"}
    for name, m in (("C2", c2), ("C4", c4)):
        greeks = [m.greek_rayleigh] + [a.greek_coefs for a in m.aerosol_optics]
        out[name] = run_leg(rtamd, m.params.polarization_type, m.quad_points.qp_μ, greeks, m.params.max_m, host_repeats)
        out[name]["model"] = run_model(rtamd, m, host_repeats)
    g = c4.aerosol_optics[0].greek_coefs
    sets = [g] + [rt.GreekCoefs(*(f * (r if q != j % 6 else -r) for q, r in enumerate((g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ))))
                  for j, f in enumerate((0.5, -0.25, 2.0, 1e-3))]
    out["C4_M32_dual"] = run_leg(rtamd, c4.params.polarization_type, c4.quad_points.qp_μ, sets, 32, host_repeats)
    out["value"] = out["C4"]["model"]["z_bases_on_device_ms"]["median"]
    out["done"] = bool(out["C2"]["model"]["device_faster_than_parent"] and out["C4"]["model"]["device_faster_than_parent"])
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    repeats = 3
    if "--host-repeats" in argv:
        i = argv.index("--host-repeats")
        repeats = int(argv[i + 1])
        del argv[i:i + 2]
    if "--resident" in argv:
        argv.remove("--resident")
        res = run_resident()
    else:
        res = run(repeats)
    if argv:
        Path(argv[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(argv[0]).write_text(json.dumps(res, indent=1, ensure_ascii=False) + "\n")
    print(json.dumps(res, ensure_ascii=False))

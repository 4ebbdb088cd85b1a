#!/usr/bin/env python3
"""The Mie / NAI-2 aerosol optics (csrc/mom_mie.hip) as a benchmark; prints one JSON line, `bench_mie.py OUT.json` also writes it
(committed as profiles/mie_bench.json).  `bench_mie.py --dual OUT.json`: the Dual run with respect to all four aerosol
parameters beside the value call in the same process (committed as profiles/mie_dual_bench.json).  `bench_mie.py --spectral
OUT.json`: 16 wavelengths in one call (mom_mie_nai2_spectral) beside 16 single calls (committed as
profiles/mie_spectral_bench.json).  `bench_mie.py --pcw OUT.json`: the Domke-PCW route (csrc/mom_pcw.hip, mom_mie_pcw) beside the
NAI-2 call at the reference's test point (committed as profiles/mie_pcw_bench.json).  `bench_mie.py --pcw-dual OUT.json`: the PCW
call with the Jacobian rows of all four aerosol parameters (mom_mie_pcw_dual) beside the value call in the same process (committed
as profiles/mie_pcw_dual_bench.json).

Two points: the reference's own test point (test/test_Scattering.jl: λ = 0.55 µm, r_max = 30 µm, nquad_radius = 2500,
m = 1.3 + 0.001i, LogNormal(log 0.3, log 6.82): x_max = 342.7, n_max = 381, n_μ = 761) and a small one (r_max = 1 µm, 37 radii:
n_max = 31, n_μ = 61).  Per point: the HIP-event times of the three kernel groups (coefficients; amplitude GEMM with its epilogue
and the reduction; projection), the wall time of the device call and of the whole compute_aerosol_optical_properties (host tables
included), and the numpy oracle of tests/mie_oracle.py on the same inputs as the CPU baseline.

Flop model of the amplitude GEMM: 16 flop per (μ, radius, l) -- S₁ and S₂, real and imaginary part, two products each.  The
achieved rate counts the K extents the kernel actually runs (per radius tile of 16: the tile's largest n_max rounded up to 4,
over all 32-row μ blocks, padding included), `algorithmic` the sums to each radius' own n_max over the n_μ live rows."""
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

PEAK_FP64_MFMA_TFLOPS = 78.6  # MI355X FP64 matrix spec
POINTS = {
    "reference_test_point": dict(lam=0.55, r_max=30.0, nquad_radius=2500, n_r=1.3, n_i=0.001, r_m=0.3, sigma_g=6.82),
    "small": dict(lam=0.55, r_max=1.0, nquad_radius=37, n_r=1.3, n_i=0.001, r_m=0.3, sigma_g=1.6),
}


def run_point(p, repeats=5, autodiff=False):
    import rtamd
    sc = rtamd.scattering
    aer = sc.Aerosol(sc.LogNormal(math.log(p["r_m"]), math.log(p["sigma_g"])), p["n_r"], p["n_i"])
    model = sc.make_mie_model(sc.NAI2(), aer, p["lam"], None, None, p["r_max"], p["nquad_radius"])
    t0 = time.perf_counter()
    inp = sc.mie_inputs(model, autodiff)
    host_ms = (time.perf_counter() - t0) * 1e3
    args = (inp.r, inp.w, p["lam"], p["n_r"], p["n_i"], inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2)
    best, call = np.full(3, 1e30), 1e30
    for _ in range(repeats + 1):      # the first call loads the code objects
        t0 = time.perf_counter()
        bulk, C, greek, ms = rtamd._lib.mie_nai2(*args)
        call = min(call, (time.perf_counter() - t0) * 1e3)
        best = np.minimum(best, ms)
    t0 = time.perf_counter()
    sc.compute_aerosol_optical_properties(model, autodiff)
    whole_ms = (time.perf_counter() - t0) * 1e3
    # K extents of the amplitude GEMM as run
    x = 2 * math.pi / p["lam"] * inp.r
    nmax = sc.get_n_max(x)
    n_mu, nR = inp.w_μ.size, inp.r.size
    tiles = [int(-(-nmax[min(i0 + 15, nR - 1)] // 4) * 4) for i0 in range(0, nR, 16)]
    flop_run = 16.0 * (-(-n_mu // 32) * 32) * 16 * float(sum(tiles))
    flop_alg = 16.0 * n_mu * float(nmax.sum())
    tf = flop_run / (best[1] * 1e-3) / 1e12
    out = {"n_radii": int(nR), "n_mu": int(n_mu), "n_max": int(nmax.max()), "x_max": float(x.max()), "weight_rows": int(inp.w.shape[0]),
           "kernels_ms": {"coefficients": float(best[0]), "amplitude_gemm_and_reduction": float(best[1]), "projection": float(best[2]),
                          "sum": float(best.sum())},
           "device_call_wall_ms": call, "host_tables_ms": host_ms, "compute_aerosol_optical_properties_wall_ms": whole_ms,
           "amplitude_gemm": {"flop_run": flop_run, "flop_algorithmic": flop_alg, "flop_full_K": 16.0 * n_mu * nR * float(nmax.max()),
                              "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                                           "frac": tf / PEAK_FP64_MFMA_TFLOPS,
                                           "algorithmic_achieved": flop_alg / (best[1] * 1e-3) / 1e12}}}
    sys.path.insert(0, str(ROOT / "tests"))
    import mie_oracle as mo
    t0 = time.perf_counter()
    o = mo.nai2_sums(inp.r, inp.w / (4 * np.pi * inp.r ** 2), p["lam"], p["n_r"], p["n_i"])
    cpu_ms = (time.perf_counter() - t0) * 1e3
    out["cpu_baseline"] = {"wall_ms": cpu_ms, "kind": "numpy oracle (tests/mie_oracle.py: vectorised recurrences, BLAS zgemm for S1, S2)",
                           "speedup_kernels": cpu_ms / float(best.sum()), "speedup_device_call": cpu_ms / call}
    out["distance_to_oracle"] = {q: mo.rel_max(g, o[q]) for q, g in (("bulk_f", bulk), ("C", C), ("greek", greek))}
    return out


def run_dual_point(p, repeats=7):
    """The Dual run (mom_mie_nai2_dual, wrt = all four parameters: three weight rows and the two index rows) beside the value call
    (mom_mie_nai2, one weight row) in the same process: the median over `repeats` calls of each call's HIP-event kernel times.
    The Dual call stands for the value call plus four more (central differences in n_r and n_i), so the criterion is
    ratio = Dual / value < 5.  Flop model of the Dual amplitude GEMM: 32 flop per (μ, radius, l) -- S and S'."""
    import rtamd
    sc = rtamd.scattering
    aer = sc.Aerosol(sc.LogNormal(math.log(p["r_m"]), math.log(p["sigma_g"])), p["n_r"], p["n_i"])
    model = sc.make_mie_model(sc.NAI2(), aer, p["lam"], None, None, p["r_max"], p["nquad_radius"])
    legs = {}
    for name, autodiff, fn in (("value", False, rtamd._lib.mie_nai2), ("dual", True, rtamd._lib.mie_nai2_dual)):
        inp = sc.mie_inputs(model, autodiff)
        args = (inp.r, inp.w, p["lam"], p["n_r"], p["n_i"], inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2)
        fn(*args)                     # the first call loads the code objects
        ms = np.array([fn(*args)[3] for _ in range(repeats)])
        med = np.median(ms, axis=0)
        legs[name] = {"weight_rows": int(inp.w.shape[0]), "repeats": repeats,
                      "kernels_ms_median": {"coefficients": float(med[0]), "amplitude_gemm_and_reduction": float(med[1]),
                                            "projection": float(med[2]), "sum": float(np.median(ms.sum(axis=1)))},
                      "kernels_ms_min_sum": float(ms.sum(axis=1).min())}
    t0 = time.perf_counter()
    sc.compute_aerosol_optical_properties(model, autodiff=True, wrt=sc.ALL_AEROSOL_PARAMETERS)
    whole_ms = (time.perf_counter() - t0) * 1e3
    x = 2 * math.pi / p["lam"] * inp.r
    nmax = sc.get_n_max(x)
    n_mu, nR = inp.w_μ.size, inp.r.size
    tiles = [int(-(-nmax[min(i0 + 15, nR - 1)] // 4) * 4) for i0 in range(0, nR, 16)]
    flop_run = 32.0 * (-(-n_mu // 32) * 32) * 16 * float(sum(tiles))
    tf = flop_run / (legs["dual"]["kernels_ms_median"]["amplitude_gemm_and_reduction"] * 1e-3) / 1e12
    ratio = legs["dual"]["kernels_ms_median"]["sum"] / legs["value"]["kernels_ms_median"]["sum"]
    return {"n_radii": int(nR), "n_mu": int(n_mu), "n_max": int(nmax.max()), "wrt": list(sc.ALL_AEROSOL_PARAMETERS), **legs,
            "ratio_dual_to_value": ratio, "criterion": "ratio_dual_to_value < 5 (a value call plus four for central differences)",
            "criterion_met": bool(ratio < 5.0), "compute_aerosol_optical_properties_wall_ms": whole_ms,
            "amplitude_gemm": {"flop_run": flop_run, "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK_FP64_MFMA_TFLOPS,
                                                                  "unit": "TFLOP/s", "frac": tf / PEAK_FP64_MFMA_TFLOPS}}}


def run_spectral_point(p, lam, repeats=5):
    """nL wavelengths at the point's radii in one spectral call: the HIP-event times of the four kernel groups (tables;
    coefficients; amplitude GEMM with reduction; projection) and the wall time of the device call, best of `repeats`; then the
    wall time of compute_spectral_aerosol_optical_properties beside nL calls of compute_aerosol_optical_properties in the same
    process (both after a first call that loads the code objects), median of three."""
    import rtamd
    sc = rtamd.scattering
    aer = sc.Aerosol(sc.LogNormal(math.log(p["r_m"]), math.log(p["sigma_g"])), p["n_r"], p["n_i"])
    model = sc.make_mie_model(sc.NAI2(), aer, p["lam"], None, None, p["r_max"], p["nquad_radius"])
    lam = np.asarray(lam, dtype=np.float64)
    n_r, n_i = np.full(lam.size, p["n_r"]), np.full(lam.size, p["n_i"])
    t0 = time.perf_counter()
    inp = sc.spectral_mie_inputs(model, lam)
    host_ms = (time.perf_counter() - t0) * 1e3
    best, call = np.full(4, 1e30), 1e30
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        ms = rtamd._lib.mie_nai2_spectral(inp.r, inp.w, lam, n_r, n_i, inp.μ, inp.w_μ, inp.n_top, inp.l_max)[3]
        call = min(call, (time.perf_counter() - t0) * 1e3)
        best = np.minimum(best, ms)
    models = [sc.make_mie_model(sc.NAI2(), aer, l, None, None, p["r_max"], p["nquad_radius"]) for l in lam]
    sc.compute_aerosol_optical_properties(models[0])
    batch, singles = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        sc.compute_spectral_aerosol_optical_properties(model, lam)
        batch.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for m in models:
            sc.compute_aerosol_optical_properties(m)
        singles.append((time.perf_counter() - t0) * 1e3)
    return {"n_wavelengths": int(lam.size), "wavelengths_um": [float(l) for l in lam], "n_radii": int(inp.r.size),
            "n_mu": int(inp.μ.size), "n_max": [int(v) for v in inp.n_max], "repeats": repeats,
            "kernels_ms": {"tables": float(best[0]), "coefficients": float(best[1]), "amplitude_gemm_and_reduction": float(best[2]),
                           "projection": float(best[3]), "sum": float(best.sum())},
            "device_call_wall_ms": call, "host_inputs_ms": host_ms,
            "compute_spectral_aerosol_optical_properties_wall_ms": {"median": float(np.median(batch)), "all": batch},
            "single_calls_wall_ms": {"median": float(np.median(singles)), "all": singles, "calls": int(lam.size)},
            "speedup_batch_over_single_calls": float(np.median(singles) / np.median(batch))}


def run_pcw_point(p, repeats=7):
    """mom_mie_pcw at the point beside mom_mie_nai2 on the same model, in the same process: the HIP-event times of the three kernel
    groups of each (median and minimum over `repeats` calls after one that loads the code objects), the wall time of the device call
    and of the public compute_aerosol_optical_properties, and the distance between the two routes' results.
    Flop model of the Gram product X~ diag(w) X~^T: the lower triangle of a (4 N) x (4 N) product over nR radii, 2 (4 N)^2 nR / 2;
    `flop_run` counts what the kernel runs (the lower triangle of 32 x 32 macro tiles of the (4 Np)^2 product, Np = N rounded up to
    16, over the radii rounded up to 16)."""
    import rtamd
    sc = rtamd.scattering
    aer = sc.Aerosol(sc.LogNormal(math.log(p["r_m"]), math.log(p["sigma_g"])), p["n_r"], p["n_i"])
    legs, optics = {}, {}
    for name, ctype in (("pcw", sc.PCW()), ("nai2", sc.NAI2())):
        model = sc.make_mie_model(ctype, aer, p["lam"], None, None, p["r_max"], p["nquad_radius"])
        if name == "pcw":
            r, wx, N = sc.pcw_inputs(model)
            call_dev = lambda: rtamd._lib.mie_pcw(r, wx, p["lam"], p["n_r"], p["n_i"], N)[2]
            groups = ("coefficients", "radius_averages", "symbols_and_sums")
        else:
            inp = sc.mie_inputs(model)
            args = (inp.r, inp.w, p["lam"], p["n_r"], p["n_i"], inp.w_μ, inp.π_, inp.τ_, inp.P, inp.P2, inp.R2, inp.T2)
            call_dev = lambda: rtamd._lib.mie_nai2(*args)[3]
            groups = ("coefficients", "amplitude_gemm_and_reduction", "projection")
        call_dev()
        ms, wall = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            ms.append(call_dev())
            wall.append((time.perf_counter() - t0) * 1e3)
        ms = np.array(ms)
        whole = []
        for _ in range(3):
            t0 = time.perf_counter()
            optics[name] = sc.compute_aerosol_optical_properties(model)
            whole.append((time.perf_counter() - t0) * 1e3)
        legs[name] = {"repeats": repeats,
                      "kernels_ms_median": {**{g: float(v) for g, v in zip(groups, np.median(ms, axis=0))}, "sum": float(np.median(ms.sum(axis=1)))},
                      "kernels_ms_min": {**{g: float(v) for g, v in zip(groups, ms.min(axis=0))}, "sum": float(ms.sum(axis=1).min())},
                      "device_call_wall_ms_median": float(np.median(wall)),
                      "compute_aerosol_optical_properties_wall_ms_median": float(np.median(whole))}
    Np, ld = -(-N // 16) * 16, -(-r.size // 16) * 16
    mrows = 4 * Np // 32
    flop_run = 2.0 * (mrows * (mrows + 1) // 2) * 32 * 32 * ld
    flop_alg = 2.0 * (4 * N) ** 2 * r.size / 2
    t = legs["pcw"]["kernels_ms_median"]["radius_averages"] * 1e-3
    rows = lambda g: (g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ)
    dist = {q: float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b)))
            for q, a, b in zip(("α", "β", "γ", "δ", "ϵ", "ζ"), rows(optics["pcw"].greek_coefs), rows(optics["nai2"].greek_coefs))}
    return {"n_radii": int(r.size), "N_max": int(N), "degrees": int(2 * N - 1), **legs,
            "radius_averages": {"note": "the group holds the diagonal sums, the Gram product and the chunk sum with the plane layout; the rate "
                                        "below divides the Gram product's flop by the time of the whole group",
                                "flop_algorithmic": flop_alg, "flop_run": flop_run,
                                "roofline": {"bound": "mfma", "achieved": flop_run / t / 1e12, "algorithmic_achieved": flop_alg / t / 1e12,
                                             "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": flop_run / t / 1e12 / PEAK_FP64_MFMA_TFLOPS}},
            "pcw_minus_nai2": {"norm2_relative": dist, "omega": float(optics["pcw"].ω̃ - optics["nai2"].ω̃),
                               "k_relative": float(optics["pcw"].k / optics["nai2"].k - 1)}}


def run_pcw():
    out = {"metric": "Mie Domke-PCW aerosol optics at the reference's test point: kernels of one call", "unit": "ms"}
    out["reference_test_point"] = run_pcw_point(POINTS["reference_test_point"])
    out["value"] = out["reference_test_point"]["pcw"]["kernels_ms_median"]["sum"]
    return out


def run_pcw_dual_point(p, repeats=7):
    """mom_mie_pcw_dual with the (r_m, σ_g) weight rows and the index rows (five output rows) beside mom_mie_pcw, alternating in one
    process: the HIP-event times of the three kernel groups (median and minimum over `repeats` calls after one that loads the code
    objects), their ratio, and the two conditions the shared work is held to -- the four-parameter call under five value calls (what
    one-sided finite differences cost), symbols_and_sums under twice the value call's (all rows share one walk over the symbols).
    Two more legs, the size rows alone and the index rows alone (three output rows each), show what a row costs in each stage.
    Flop model of the Gram products, as run: three weight rows on the lower triangle of 32 x 32 macro tiles and the index rows'
    non-symmetric product on the full square, each over the radii rounded up to 16; the rate divides by the whole radius_averages
    group (diagonal sums, products, chunk sums)."""
    import rtamd
    sc = rtamd.scattering
    aer = sc.Aerosol(sc.LogNormal(math.log(p["r_m"]), math.log(p["sigma_g"])), p["n_r"], p["n_i"])
    model = sc.make_mie_model(sc.PCW(), aer, p["lam"], None, None, p["r_max"], p["nquad_radius"])
    r, w, N, index_rows, _ = sc.pcw_jacobian_inputs(model, sc.ALL_AEROSOL_PARAMETERS)
    dual = lambda rows, index: rtamd._lib.mie_pcw_dual(r, rows, p["lam"], p["n_r"], p["n_i"], N, index_rows=index)[2]
    calls = {"value": lambda: rtamd._lib.mie_pcw(r, w[0], p["lam"], p["n_r"], p["n_i"], N)[2],
             "four_parameters": lambda: dual(w, index_rows),
             "size_rows_only": lambda: dual(w, False),         # three output rows: w_x and its (r_m, σ_g) rows
             "index_rows_only": lambda: dual(w[:1], True)}     # three output rows: w_x and its (nᵣ, nᵢ) rows
    groups = ("coefficients", "radius_averages", "symbols_and_sums")
    ms, wall = {k: [] for k in calls}, {k: [] for k in calls}
    for c in calls.values():
        c()
    for _ in range(repeats):
        for k, c in calls.items():
            t0 = time.perf_counter()
            ms[k].append(c())
            wall[k].append((time.perf_counter() - t0) * 1e3)
    legs = {}
    for k in calls:
        m = np.array(ms[k])
        legs[k] = {"repeats": repeats,
                   "kernels_ms_median": {**{g: float(v) for g, v in zip(groups, np.median(m, axis=0))}, "sum": float(np.median(m.sum(axis=1)))},
                   "kernels_ms_min": {**{g: float(v) for g, v in zip(groups, m.min(axis=0))}, "sum": float(m.sum(axis=1).min())},
                   "device_call_wall_ms_median": float(np.median(wall[k]))}
    whole = []
    for _ in range(3):
        t0 = time.perf_counter()
        sc.aerosol_optics_jacobian(model)
        whole.append((time.perf_counter() - t0) * 1e3)
    v, d = legs["value"]["kernels_ms_median"], legs["four_parameters"]["kernels_ms_median"]
    ratio = {g: d[g] / v[g] for g in groups + ("sum",)}
    Np, ld = -(-N // 16) * 16, -(-r.size // 16) * 16
    mrows = 4 * Np // 32
    flop_run = 2.0 * (3 * (mrows * (mrows + 1) // 2) + mrows * mrows) * 32 * 32 * ld
    t = d["radius_averages"] * 1e-3
    conditions = {"four_parameters_under_five_value_calls": bool(d["sum"] < 5 * v["sum"]),
                  "symbols_and_sums_under_twice_the_value_calls": bool(d["symbols_and_sums"] < 2 * v["symbols_and_sums"])}
    over = [g for g in groups if d[g] >= (2 if g == "symbols_and_sums" else 5) * v[g]]
    return {"n_radii": int(r.size), "N_max": int(N), "degrees": int(2 * N - 1), "output_rows": int(w.shape[0] + 2), **legs,
            "aerosol_optics_jacobian_wall_ms_median": float(np.median(whole)),
            "four_parameters_over_value": ratio, "conditions": conditions, "stages_over": over,
            "radius_averages": {"flop_run": flop_run,
                                "roofline": {"bound": "mfma", "achieved": flop_run / t / 1e12, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                                             "frac": flop_run / t / 1e12 / PEAK_FP64_MFMA_TFLOPS}}}


def run_pcw_dual():
    out = {"metric": "Mie Domke-PCW aerosol optics with the Jacobian rows of (r_m, σ_g, nᵣ, nᵢ) at the reference's test point: kernels "
                     "of one call", "unit": "ms"}
    out["reference_test_point"] = run_pcw_dual_point(POINTS["reference_test_point"])
    out["value"] = out["reference_test_point"]["four_parameters"]["kernels_ms_median"]["sum"]
    return out


def run_spectral():
    out = {"metric": "Mie NAI-2 aerosol optics, 16 wavelengths (0.4 .. 2.2 µm) in one spectral call: wall time of the public call",
           "unit": "ms"}
    out["reference_test_point"] = run_spectral_point(POINTS["reference_test_point"], np.linspace(0.4, 2.2, 16))
    out["value"] = out["reference_test_point"]["compute_spectral_aerosol_optical_properties_wall_ms"]["median"]
    return out


def run():
    out = {"metric": "Mie NAI-2 aerosol optics, kernels of one call", "unit": "ms"}
    for name, p in POINTS.items():
        out[name] = run_point(p)
    out["reference_test_point_nW3"] = run_point(POINTS["reference_test_point"], autodiff=True)
    out["value"] = out["reference_test_point"]["kernels_ms"]["sum"]
    return out


def run_dual():
    out = {"metric": "Mie NAI-2 aerosol optics, Dual run with respect to (r_m, σ_g, nᵣ, nᵢ): kernels of one call", "unit": "ms"}
    out["reference_test_point"] = run_dual_point(POINTS["reference_test_point"])
    out["value"] = out["reference_test_point"]["dual"]["kernels_ms_median"]["sum"]
    return out


if __name__ == "__main__":
    argv = [a for a in sys.argv[1:] if a not in ("--dual", "--spectral", "--pcw", "--pcw-dual")]
    if "--pcw-dual" in sys.argv[1:]:
        res = run_pcw_dual()
    elif "--pcw" in sys.argv[1:]:
        res = run_pcw()
    else:
        res = run_dual() if "--dual" in sys.argv[1:] else (run_spectral() if "--spectral" in sys.argv[1:] else run())
    if argv:
        Path(argv[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(argv[0]).write_text(json.dumps(res, indent=1, ensure_ascii=False) + "\n")
    print(json.dumps(res, ensure_ascii=False))

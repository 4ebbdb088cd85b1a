#!/usr/bin/env python3
"""The δ-BGE truncation on the device (csrc/mom_trunc.hip, mom_truncate_phase) as a benchmark; prints one JSON line,
`bench_truncate.py OUT.json` also writes it (committed as profiles/truncate_bench.json).  `--host-repeats R` (default 3): runs of
each host timing.

Two shapes.  (a) The band set-up of scenes.make_mie_band_scene: its default aerosol (r_m = 0.3, σ_g = 1.6, 1.3 + 0.001i, r_max = 1,
37 radii) at the three band centres 0.76, 1.6 and 2.06 µm, δBGE(33): what band_aerosol_optics truncates, values only and with the
four partials of ALL_AEROSOL_PARAMETERS.  The three sets have three lengths (2 n_max(λ) - 1 = 51, 39, 37 terms, n_μ = l_full each), so
the device route makes three calls.  (b) The reference's Mie test point (λ = 0.55, r_max = 30, 2500 radii, LogNormal(log 0.3,
log 6.82): n_μ = l_full = 761), δBGE(121), four partials, for 1 and for 16 sets.  Per leg: the wall time of the host loop over
truncate_phase (median), of the device route (truncate_phase_batch(device=0) per length; median of 5 after a first call that loads the code objects) and the
HIP-event time of the kernels (best of 5), and the largest distance of the device's rows to the host's relative to each row's
largest magnitude (the two differ by the host's own error).  The Mie sums themselves are not timed."""
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))


def _median_ms(f, repeats):
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), t


def _rows(o):
    g = o.greek_coefs
    return np.array([g.α, g.β, g.γ, g.δ, g.ϵ, g.ζ])


def _distance(dev, host):
    """largest |device - host| over the truncated sets and their partials, per Greek row relative to the row's largest magnitude"""
    worst = 0.0
    for d, h in zip(dev, host):
        pairs = [(d, h)] if not isinstance(d, tuple) else [(d[0], h[0])] + list(zip(d[1], h[1]))
        for a, b in pairs:
            ra, rb = _rows(a), _rows(b)
            top = np.max(np.abs(rb), axis=1)
            worst = max(worst, float(np.max(np.max(np.abs(ra - rb), axis=1)[top > 0] / top[top > 0])))
    return worst


def run_leg(rtamd, mod, optics, partials, host_repeats, device_repeats=5):
    sc, L = rtamd.scattering, rtamd._lib
    lengths = [len(o.greek_coefs.β) for o in optics]
    nP = 0 if partials is None else len(partials[0])
    kernels_ms = 0.0
    for l_full in sorted(set(lengths)):   # one device call per distinct length, as the public layer makes them
        idx = [i for i, n in enumerate(lengths) if n == l_full]
        greek = np.array([[_rows(a) for a in [optics[i]] + (partials[i] if partials is not None else [])] for i in idx])
        μ, w_μ = sc.gausslegendre(l_full)
        ms = [L.truncate_phase(μ, w_μ, greek, mod.l_max)[3] for _ in range(device_repeats + 1)]   # the first call loads the code objects
        kernels_ms += min(ms[1:])
    dev = {}
    dev_ms, dev_all = _median_ms(lambda: dev.update(r=sc._truncate_grouped(mod, optics, partials, 0)), device_repeats)
    host = {}
    host_ms, host_all = _median_ms(lambda: host.update(r=sc._truncate_grouped(mod, optics, partials, None)), host_repeats)
    return {"sets": len(optics), "partials": nP, "l_full": lengths, "device_calls": len(set(lengths)), "l_tr": int(mod.l_max), "kernels_ms": kernels_ms,
            "device_call_wall_ms": {"median": dev_ms, "runs": dev_all}, "host_loop_wall_ms": {"median": host_ms, "runs": host_all},
            "speedup_public_call": host_ms / dev_ms, "device_faster_than_host": bool(dev_ms < host_ms),
            "max_rel_device_minus_host": _distance(dev["r"], host["r"])}


def run(host_repeats=3):
    import rtamd
    sc = rtamd.scattering
    out = {"metric": "δ-BGE truncation of 16 Greek sets with four partials at the reference's Mie test point (l_full = 761, l_tr = 121): "
                     "wall time of truncate_phase_batch on the device", "unit": "ms"}
    wrt = sc.ALL_AEROSOL_PARAMETERS
    # (a) the band set-up
    aer = sc.Aerosol(sc.LogNormal(math.log(0.3), math.log(1.6)), 1.3, 0.001)
    mie = sc.make_mie_model(sc.NAI2(), aer, 0.76, rtamd.Stokes_IQU(), sc.δBGE(33, 2.0), 1.0, 37)
    raw, parts = sc.compute_spectral_aerosol_optical_properties(mie, np.array([0.76, 1.6, 2.06]), autodiff=True, wrt=wrt)
    out["bands_values"] = run_leg(rtamd, mie.truncation_type, raw, None, host_repeats)
    out["bands_four_partials"] = run_leg(rtamd, mie.truncation_type, raw, parts, host_repeats)
    # (b) the reference's test point
    aer = sc.Aerosol(sc.LogNormal(math.log(0.3), math.log(6.82)), 1.3, 0.001)
    mie = sc.make_mie_model(sc.NAI2(), aer, 0.55, rtamd.Stokes_IQU(), sc.δBGE(121, 2.0), 30.0, 2500)
    aero, part = sc.compute_aerosol_optical_properties(mie, autodiff=True, wrt=wrt)
    out["test_point_1_set"] = run_leg(rtamd, mie.truncation_type, [aero], [part], host_repeats)
    out["test_point_16_sets"] = run_leg(rtamd, mie.truncation_type, [aero] * 16, [part] * 16, host_repeats)
    out["value"] = out["test_point_16_sets"]["device_call_wall_ms"]["median"]
    out["done"] = True
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    repeats = 3
    if "--host-repeats" in argv:
        i = argv.index("--host-repeats")
        repeats = int(argv[i + 1])
        del argv[i:i + 2]
    res = run(repeats)
    if argv:
        Path(argv[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(argv[0]).write_text(json.dumps(res, indent=1, ensure_ascii=False) + "\n")
    print(json.dumps(res, ensure_ascii=False))

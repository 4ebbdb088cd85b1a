#!/usr/bin/env python3
"""From the resident dτ_abs table to the scene's partials at the C2 shape (S = 10 000, Nz = 40, one aerosol type: K = 2, P = 3), by the
two routes:
  (a) the host route: absorption_get_partials (device -> host of [S, Nz, 2]) + absorption.optics_partials (numpy) +
      corert.scene_set_partials (pack, upload of dτ, dϖ [S, Nz, P]);
  (b) the device route: corert.scene_set_optics_partials (k_optics_dual forms dτ, dϖ, dzw in the buffers mom_rt_run_dual reads).
Both end in a device synchronise; wall time per route, alternating, after a warm-up; the kernel's time from HIP events (mom_timers
right after the call); achieved bytes/s = (bytes written + bytes read) / kernel time, with the bytes counted from the shapes here.
The three parameters act through the gas absorption only (a uniform temperature offset, a uniform relative pressure change, a
temperature offset of the lower half), the one kind route (a) covers.  Writes profiles/optics_dual_timing.json and prints it.
A measuring tool, not a test and not part of bench.py."""
import argparse
import dataclasses
import json
import statistics
import sys
import time
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import rtamd  # noqa: E402


def kernel_bytes(S, Nz, K, P, dzw):
    """what k_optics_dual moves: (2 + K) S Nz P doubles written (2 without dzw); τ_rayl, τ_abs and the two dτ_abs tables read, once
    (the least the algorithm needs) or once per partial (what the threads request; the repeats can hit in the caches)"""
    written = (2 + (K if dzw else 0)) * S * Nz * P * 8
    return written, 4 * S * Nz * 8, 4 * S * Nz * P * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=10_000)
    ap.add_argument("--Nz", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "optics_dual_timing.json"))
    a = ap.parse_args()
    ab, rt = rtamd.absorption, rtamd.corert
    S, Nz = a.S, a.Nz
    base = rtamd.scenes.scene_C2(S, Nz)
    grid = np.linspace(12903.0, 13245.0, S)
    p_half = rtamd.scenes.pressure_grid(Nz)
    p_full = 0.5 * (p_half[1:] + p_half[:-1])
    T = 216.0 + (288.0 - 216.0) * (p_full / 1000.0) ** 0.19
    vcd = 2.0e25 * np.diff(p_half) / p_half[-1]
    lower = (np.arange(Nz) >= Nz // 2).astype(np.float64)
    ps = [rt.OpticsPartial(w_T=np.ones(Nz)), rt.OpticsPartial(w_p=p_full.copy()), rt.OpticsPartial(w_T=lower)]
    P, K = len(ps), 1 + len(base.aerosol_optics)
    with rt.make_handle(base) as h:
        ab.compute_absorption_profile(h, ab.synthetic_o2a_lines(300), grid, p_full, T, vcd, 0.21, wing_cutoff=40.0, model_vmr=0.21,
                                      device_prefactors=True, dual=True)
        model = dataclasses.replace(base, τ_abs=h.absorption_get())
        kind = rt.scene_set_device_optics(h, model, upload_tau_abs=False)
        _, _, tau, varpi, _, _ = h.scene_get_layers(Nz, K)
        τ, ϖ = tau.reshape(Nz, S).T, varpi.reshape(Nz, S).T          # route (a) starts from the scene's τ, ϖ on the host
        sc = types.SimpleNamespace(surf_kind=kind)                   # all corert.scene_set_partials reads of the scene

        def route_a():
            d = h.absorption_get_partials()
            parts = [ab.optics_partials(τ, ϖ, d[1]), ab.optics_partials(τ, ϖ, d[0] * p_full[None, :]), ab.optics_partials(τ, ϖ, d[1] * lower[None, :])]
            rt.scene_set_partials(h, sc, parts)

        def route_b():
            rt.scene_set_optics_partials(h, model, ps, surf_kind=kind)

        wall = {"a": [], "b": []}
        kern = []
        got = {}
        for it in range(a.warmup + a.repeats):
            for name, fn in (("a", route_a), ("b", route_b)):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if it >= a.warmup:
                    wall[name].append(dt * 1e3)
                    if name == "b":
                        kern.append(float(h.timers()["total_ms"]))
                if it == 0:
                    got[name] = h.scene_get_partials()
        # the kernel at its full width: one parameter also moves the Rayleigh depth, so dzw [K, S, Nz, P] is formed and stored too
        wide = [dataclasses.replace(ps[0], w_rayl=np.ones(Nz))] + ps[1:]
        kern_wide = []
        for it in range(a.warmup + a.repeats):
            rt.scene_set_optics_partials(h, model, wide, surf_kind=kind)
            if it >= a.warmup:
                kern_wide.append(float(h.timers()["total_ms"]))
    # the two routes hold the same partials (route (a) has no dzw: it reads as zeros, and the device route's is absent as well)
    worst = 0.0
    for x, y in zip(got["a"], got["b"]):
        scale = np.abs(x).max(axis=1, keepdims=True) if x.ndim == 3 else 1.0
        worst = max(worst, float(np.max(np.abs(x - y) / np.where(scale > 0, scale, 1.0))))
    assert worst <= 1e-12, worst
    written, read_once, read_req = kernel_bytes(S, Nz, K, P, dzw=False)
    k_ms = statistics.median(kern)
    out = {"shape": {"S": S, "Nz": Nz, "K": K, "P": P}, "repeats": a.repeats, "warmup": a.warmup,
           "route_a_host_ms": {"median": statistics.median(wall["a"]), "min": min(wall["a"]), "max": max(wall["a"])},
           "route_b_device_ms": {"median": statistics.median(wall["b"]), "min": min(wall["b"]), "max": max(wall["b"])},
           "route_a_over_b": statistics.median(wall["a"]) / statistics.median(wall["b"]),
           "k_optics_dual_ms": {"median": k_ms, "min": min(kern), "max": max(kern)},
           "kernel_bytes": {"written": written, "read_once": read_once, "read_requested": read_req},
           "kernel_bytes_per_s": (written + read_once) / (k_ms * 1e-3),
           "kernel_bytes_per_s_requested": (written + read_req) / (k_ms * 1e-3),
           "routes_agree_to": worst}
    w_written, _, w_req = kernel_bytes(S, Nz, K, P, dzw=True)
    kw_ms = statistics.median(kern_wide)
    out["with_dzw"] = {"k_optics_dual_ms": {"median": kw_ms, "min": min(kern_wide), "max": max(kern_wide)},
                       "kernel_bytes": {"written": w_written, "read_once": read_once, "read_requested": w_req},
                       "kernel_bytes_per_s": (w_written + read_once) / (kw_ms * 1e-3),
                       "kernel_bytes_per_s_requested": (w_written + w_req) / (kw_ms * 1e-3)}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

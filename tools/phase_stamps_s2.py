"""Timelines of the two-buffer strip image (csrc/mom_strip2.hpp) on a C2 run: MOM_LIBRARY must point at a library whose
momcore_s2s15.o was built with -DMOM_DIAG_TIMELINE (tools/build_variant_fast.sh tl2 -DMOM_DIAG_TIMELINE momcore_s2s15.o).
Every workgroup logs, on the common 100 MHz clock, when each of its sections ended (from its second unit on).  For every CU that
hosts two workgroups the two timelines are laid over each other on their common interval; printed per MOM_OPT_STRIP2_SCHED setting:
the share per section (mean over workgroups; favoured and other workgroups apart) and the share of time in which both units, one
unit, or no unit is inside a strip chain.  usage: python tools/phase_stamps_s2.py [sched values, default 0 3]"""
import sys, os, ctypes as C
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ["MOM_LIBRARY"] = os.environ.get("MOM_LIBRARY", os.path.join(ROOT, "scratch", "ab", "lib_tl2.so"))
if not os.path.exists(os.environ["MOM_LIBRARY"]):
    sys.exit(f"{os.environ['MOM_LIBRARY']}: no such library -- build it first: "
             "tools/build_variant_fast.sh tl2 -DMOM_DIAG_TIMELINE momcore_s2s15.o (or point MOM_LIBRARY at a timeline build)")
import numpy as np
import rtamd

SEC = ["unit top", "elemental layer", "doubling steps (chain)", "doubling: apply D", "int: R+- copy (a)", "int: chains (a)-(c)",
       "int: T++ copy (d)", "int: products with T++ (chain)", "int: final barrier", "first layer store"]
CHAIN = (2, 5, 7)
model = rtamd.scenes.scene_C2(S=int(os.environ.get("S2_POINTS", "10000")))
sc = rtamd.prepare_scene(model)
lib = rtamd._lib.load()
rd = lib.mom2_strip15_timeline_read
rd.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_int)]
wgs, cap = C.c_int(), C.c_int()
rd(None, None, C.byref(wgs), C.byref(cap))
wgs, cap = wgs.value, cap.value
ev = (C.c_ulonglong * (wgs * cap))()
hdr = (C.c_uint * (4 * wgs))()


def intervals(e):
    """(start, end, in_chain) per logged section of one workgroup"""
    t, sid = (e >> np.uint64(4)).astype(np.int64), (e & np.uint64(15)).astype(int)
    return t[:-1], t[1:], np.isin(sid[1:], CHAIN), sid[1:]


def overlap(a, b):
    """shares of [max start, min end] in which 2, 1, 0 of the two workgroups are inside a chain (sweep over the merged breakpoints)"""
    lo, hi = max(a[0][0], b[0][0]), min(a[1][-1], b[1][-1])
    if hi <= lo:
        return None
    pts = np.unique(np.concatenate([a[0], a[1], b[0], b[1], [lo, hi]]))
    pts = pts[(pts >= lo) & (pts <= hi)]
    mid = (pts[:-1] + pts[1:]) / 2.0
    w = np.diff(pts).astype(float)
    ina = a[2][np.clip(np.searchsorted(a[1], mid), 0, len(a[1]) - 1)]
    inb = b[2][np.clip(np.searchsorted(b[1], mid), 0, len(b[1]) - 1)]
    k = ina.astype(int) + inb.astype(int)
    return np.array([w[k == 2].sum(), w[k == 1].sum(), w[k == 0].sum()]) / w.sum()


for sched in [int(x) for x in (sys.argv[1:] or ["0", "3"])]:
    with rtamd.corert.make_handle(model) as h:
        h.set_option(rtamd._lib.MOM_OPT_STRIP2_SCHED, sched)
        rtamd.corert.run_scene(h, sc)
        rtamd.corert.run_scene(h, sc)
        assert rd(ev, hdr, C.byref(C.c_int()), C.byref(C.c_int())) == 0
    E = np.frombuffer(ev, dtype=np.uint64).reshape(wgs, cap)
    H = np.frombuffer(hdr, dtype=np.uint32).reshape(wgs, 4)
    iv = {b: intervals(E[b, :H[b, 3]]) for b in range(wgs) if H[b, 3] > 16}
    print(f"== MOM_OPT_STRIP2_SCHED = {sched}: {len(iv)} workgroups with a timeline, {len(set(H[list(iv), 0]))} CUs")
    for fav in (0, 1):
        sel = [b for b in iv if H[b, 2] == fav]
        if not sel:
            continue
        sh = np.zeros(len(SEC))
        for b in sel:
            s, e, _, sid = iv[b]
            sh += np.bincount(sid, weights=(e - s).astype(float), minlength=len(SEC))[:len(SEC)] / float(e[-1] - s[0])
        sh /= len(sel)
        print(f"-- {'favoured' if fav else 'other'} workgroups ({len(sel)}): share of the logged time per section; in chains {100 * sh[list(CHAIN)].sum():.1f} %")
        for k in np.argsort(-sh):
            if sh[k] > 0:
                print(f"   {SEC[k]:34s} {100 * sh[k]:6.2f} %")
    bycu = {}
    for b in iv:
        bycu.setdefault(int(H[b, 0]), []).append(b)
    ov = [o for o in (overlap(iv[v[0]], iv[v[1]]) for v in bycu.values() if len(v) == 2) if o is not None]
    if ov:
        ov = np.array(ov)
        m, sd = ov.mean(0), ov.std(0)
        print(f"-- {len(ov)} CUs with two workgroups, on their common interval: both in a chain {100 * m[0]:.1f} % (sd {100 * sd[0]:.1f}), "
              f"one {100 * m[1]:.1f} % (sd {100 * sd[1]:.1f}), BOTH OUTSIDE {100 * m[2]:.1f} % (sd {100 * sd[2]:.1f})")
    print(f"   CUs by number of workgroups: { {n: sum(1 for v in bycu.values() if len(v) == n) for n in (1, 2, 3, 4)} }")

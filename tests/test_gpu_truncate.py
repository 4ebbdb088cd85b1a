"""mom_truncate_phase and the public layer on top of it (truncate_phase(device=), truncate_phase_batch, band_aerosol_optics(device=))
against the longdouble arbiter under the rule of trunc_cases.py, at the shapes where the kernels change form: empty, 1 x 1 and 2 x 2
γ / ϵ fits (l_tr = 1 .. 4), the MFMA tile and 64-tile edges for both l_tr and l_tr - 2, an odd node count (k-step remainder),
l_tr = l_full, the largest order 128, n_μ != l_full, batches, and the status word of a set whose f₁₂ is zero by construction."""
import numpy as np
import pytest

import trunc_cases as tc
import trunc_oracle as to

pytestmark = pytest.mark.gpu

SHAPES = [("case2", l) for l in (1, 2, 3, 4, 15, 16, 17, 32, 33, 60, 61)] + [("absorbing", 41)] + [("bigger", l) for l in (64, 65, 66, 121, 128)]


def _pack(g, dirs):
    return np.concatenate([g[None], dirs])[None]     # [1, 1 + nP, 6, l_full]


@pytest.mark.parametrize("case,l_tr", SHAPES)
def test_values_and_partials_against_arbiter(rtamd, case, l_tr):
    """nP = 0, 1, 2, 4 on gausslegendre(l_full); the arbiter and the host run once with four partials, whose first rows are those
    of the shorter runs (every partial is differentiated by itself)"""
    L, sc = rtamd._lib, rtamd.scattering
    g, dirs = tc.greek_set(case)
    ref = tc.arbiter(case, l_tr, 4)
    hg, hc = tc.host_arrays(rtamd, l_tr, g, dirs)
    μ, w = sc.gausslegendre(g.shape[1])
    report = []
    for nP in (0, 1, 2, 4):
        gt, c0, status, ms = L.truncate_phase(μ, w, _pack(g, dirs[:nP]), l_tr)
        assert not status.any() and ms > 0.0
        sub = dict(greek=ref["greek"][:1 + nP], c0=ref["c0"][:1 + nP], kappa=ref["kappa"])
        tc.check(f"{case} l_tr={l_tr} nP={nP}", gt[0], c0[0], hg[:1 + nP], hc[:1 + nP], sub, l_tr, report if nP == 4 else None)
    worst = max(report, key=lambda r: r[2] / r[4])
    print(f"{case} l_tr={l_tr}: κ = {ref['kappa']}, worst field {worst[1]}: device {worst[2]:.2e}, host {worst[3]:.2e}, allowed {worst[4]:.2e}; "
          f"largest device distance {max(r[2] for r in report):.2e}")


@pytest.mark.parametrize("n_mu", [64, 67])
def test_node_count_free_of_l_full(rtamd, n_mu):
    """through the C call: case2's 61 terms on 64 and 67 nodes (host: the numpy text on the same nodes)"""
    L, sc = rtamd._lib, rtamd.scattering
    g, dirs = tc.greek_set("case2")
    for l_tr in (17, 33):
        ref = tc.arbiter("case2", l_tr, 2, None, n_mu)
        hg, hc = tc.host_arrays(rtamd, l_tr, g, dirs[:2], n_mu=n_mu)
        gt, c0, status, _ = L.truncate_phase(*sc.gausslegendre(n_mu), _pack(g, dirs[:2]), l_tr)
        assert not status.any()
        tc.check(f"case2 on {n_mu} nodes, l_tr={l_tr}", gt[0], c0[0], hg, hc, ref, l_tr)


def test_batches_are_their_sets_bitwise(rtamd):
    """nG = 1, 3, 17 with the three cases interleaved, zero-padded to l_full = 129: each set's rows are bitwise those of its own
    single-set call and within max(4 κ 2⁻⁵², 2⁻⁴⁶) of its (padded) arbiter; two identical calls are bitwise equal"""
    L, sc = rtamd._lib, rtamd.scattering
    names, l_tr, nP, l_full = sorted(tc.CASES), 33, 2, 129
    μ, w = sc.gausslegendre(l_full)
    packed = {n: _pack(tc.greek_set(n, l_full)[0], tc.greek_set(n, l_full)[1][:nP]) for n in names}
    single = {n: L.truncate_phase(μ, w, packed[n], l_tr) for n in names}
    for n in names:   # the host stands up to 7.6e-6 from the arbiter at these padded sets (case2's γ fit): the rule without its host term
        print(n, tc.check(f"{n} padded to {l_full}", single[n][0][0], single[n][1][0], None, None, tc.arbiter(n, l_tr, nP, l_full), l_tr))
    for nG in (1, 3, 17):
        order = [names[i % 3] for i in range(nG)]
        batch = np.concatenate([packed[n] for n in order])
        a, b = L.truncate_phase(μ, w, batch, l_tr), L.truncate_phase(μ, w, batch, l_tr)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not a[2].any()
        for i, n in enumerate(order):
            assert np.array_equal(a[0][i], single[n][0][0]) and np.array_equal(a[1][i], single[n][1][0]), (nG, i, n)


def test_status_word_of_a_singular_set(rtamd):
    """set 1 of three has γ ≡ 0, so f₁₂ ≡ 0: a divisor that is zero by construction.  MOM_ESINGULAR names set 1 and fit 1, its rows
    are NaN, the other sets are bitwise their single-set results, and the public layer raises LinAlgError."""
    L, sc, lib = rtamd._lib, rtamd.scattering, rtamd.load()
    l_tr = 17
    g, dirs = tc.greek_set("case2")
    g2, dirs2 = tc.greek_set("absorbing", g.shape[1])
    flat = g.copy()
    flat[2] = 0.0
    μ, w = sc.gausslegendre(g.shape[1])
    batch = np.concatenate([_pack(g, dirs[:1]), _pack(flat, dirs[:1]), _pack(g2, dirs2[:1])])
    out, c0, status, ms = np.zeros((3, 2, 6, l_tr)), np.zeros((3, 2)), np.zeros(3, dtype=np.int32), np.zeros(1)
    rc = lib.mom_truncate_phase(0, len(μ), L.dp(μ), L.dp(w), 3, 1, g.shape[1], l_tr, L.dp(L.f64(batch)), L.dp(out), L.dp(c0), L.ip(status),
                                L.dp(ms))
    msg = lib.mom_last_global_error()
    assert rc == L.MOM_ESINGULAR and b"set 1, fit 1" in msg, (rc, msg)
    assert list(status) == [0, 2, 0]
    assert np.all(np.isnan(out[1])) and np.all(np.isnan(c0[1]))
    for i, one in ((0, _pack(g, dirs[:1])), (2, _pack(g2, dirs2[:1]))):
        gt, cc, st, _ = L.truncate_phase(μ, w, one, l_tr)
        assert not st.any() and np.array_equal(gt[0], out[i]) and np.array_equal(cc[0], c0[i]), i
    wrapped = L.truncate_phase(μ, w, batch, l_tr)          # the wrapper hands the status words on
    assert list(wrapped[2]) == [0, 2, 0] and np.array_equal(wrapped[0][[0, 2]], out[[0, 2]])
    sets = [tc.optics(rtamd, x) for x in (g, flat, g2)]
    with pytest.raises(np.linalg.LinAlgError, match="set 1, fit 1"):
        rtamd.truncate_phase_batch(sc.δBGE(l_tr, 2.0), sets)


def test_public_layer_against_host_route(rtamd):
    """truncate_phase(device=0) and truncate_phase_batch against the numpy route, the arbiter between them"""
    sc = rtamd.scattering
    mod = sc.δBGE(17, 2.0)
    sets, parts, refs, hosts = [], [], [], []
    for n, nP in (("case2", 4), ("absorbing", 0)):
        g, dirs = tc.greek_set(n, 61)
        sets.append(tc.optics(rtamd, g))
        parts.append([tc.optics(rtamd, d) for d in dirs[:nP]])
        refs.append(tc.arbiter(n, 17, nP, 61))
        hosts.append(tc.from_optics(sc.truncate_phase(mod, sets[-1], parts[-1])))
    one = sc.truncate_phase(mod, sets[0], parts[0], device=0)
    tc.check("truncate_phase(device=0)", *tc.from_optics(one), *hosts[0], refs[0], 17)
    assert (one[0].ω̃, one[0].k) == (sets[0].ω̃, sets[0].k) and [(p.ω̃, p.k) for p in one[1]] == [(p.ω̃, p.k) for p in parts[0]]
    plain = sc.truncate_phase(mod, sets[0], device=0)
    assert np.array_equal(tc.stack(plain), tc.stack(one[0])) and plain.fᵗ == one[0].fᵗ
    batch = rtamd.truncate_phase_batch(mod, sets, parts)       # a set with four partials and one with none in one call
    assert np.array_equal(tc.from_optics(batch[0])[0], tc.from_optics(one)[0]) and batch[1][1] == []
    tc.check("batch set 1", *tc.from_optics(batch[1]), *hosts[1], refs[1], 17)
    values = rtamd.truncate_phase_batch(mod, sets)
    assert all(np.array_equal(tc.stack(v), tc.stack(b[0])) and v.fᵗ == b[0].fᵗ for v, b in zip(values, batch))


def test_band_aerosol_optics_on_the_device(rtamd):
    """the smallest band set-up of bands_cases.py (l_trunc 5, Nz 3, its aerosol column as the profile) with a Mie aerosol in three
    bands, autodiff over all four parameters: the bands of one Greek-set length (the first two) share ONE device call.  Optics and d_optics against the
    device=None result under the rule; τ_aer and dτ_aer are formed from k, which passes through on the host: bitwise."""
    import bands_cases as bc
    sc = rtamd.scattering
    base = bc.base_scene(78, 1)
    τ_ref = float(base.τ_aer.sum())
    profile, λ_bands, λ_ref = base.τ_aer[0] / τ_ref, np.array([0.76, 0.765, 1.6]), 0.55
    l_tr = base.params.l_trunc
    mie = sc.make_mie_model(sc.NAI2(), sc.Aerosol(sc.LogNormal(np.log(0.3), np.log(1.6)), 1.3, 0.001), λ_ref, rtamd.Stokes_IQU(),
                            sc.δBGE(l_tr, 2.0), 1.0, 37)
    wrt = sc.ALL_AEROSOL_PARAMETERS
    calls = []
    real = rtamd._lib.truncate_phase
    rtamd._lib.truncate_phase = lambda *a, **k: (calls.append(a[2].shape), real(*a, **k))[1]
    try:
        dev = sc.band_aerosol_optics(mie, λ_bands, λ_ref, τ_ref, profile, autodiff=True, wrt=wrt, device=0)
        dev_values = sc.band_aerosol_optics(mie, λ_bands, λ_ref, τ_ref, profile, device=0)
    finally:
        rtamd._lib.truncate_phase = real
    host = sc.band_aerosol_optics(mie, λ_bands, λ_ref, τ_ref, profile, autodiff=True, wrt=wrt)
    raw, parts = sc.compute_spectral_aerosol_optical_properties(mie, np.append(λ_bands, λ_ref), autodiff=True, wrt=wrt)
    assert sorted(c[:3] for c in calls) == [(1, 1, 6), (1, 1 + len(wrt), 6), (2, 1, 6), (2, 1 + len(wrt), 6)]
    assert len({len(o.greek_coefs.β) for o in raw[:3]}) == 2
    assert np.array_equal(dev[1], host[1]) and np.array_equal(dev[3], host[3]) and np.array_equal(dev_values[1], host[1])
    for b in range(3):
        ref = to.truncate(l_tr, tc.stack(raw[b]), [tc.stack(p) for p in parts[b]])
        tc.check(f"band {b}", *tc.from_optics((dev[0][b], dev[2][b])), *tc.from_optics((host[0][b], host[2][b])), ref, l_tr)
        assert (dev[0][b].ω̃, dev[0][b].k) == (host[0][b].ω̃, host[0][b].k)
        assert [(p.ω̃, p.k) for p in dev[2][b]] == [(p.ω̃, p.k) for p in host[2][b]]
        assert np.array_equal(tc.stack(dev_values[0][b]), tc.stack(dev[0][b])) and dev_values[0][b].fᵗ == dev[0][b].fᵗ

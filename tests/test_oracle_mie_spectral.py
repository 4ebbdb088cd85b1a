"""The cases of the spectral Mie call (tests/mie_spectral_cases.py) on the CPU: every case reaches the edges it was laid out for,
scattering.spectral_mie_inputs chooses the grid of the shortest wavelength, and the comparison rule the GPU tests use tells the
wavelengths of a batch apart.  The device is checked in test_gpu_mie_spectral.py."""
import numpy as np

import mie_oracle as mo
import mie_shapes as ms
import mie_spectral_cases as sc


def test_base_case_conditions():
    tile_r, mu_block, k_step, _ = ms.kernel_constants()
    case = sc.BASE
    n_max = sc.n_max_per_wavelength(case)
    assert np.all(np.diff(n_max, axis=1) >= 0)
    assert [int(v) for v in n_max[:, -1]] == [39, 31, 19]           # the shorter tables run with 8 and 20 spare rows
    assert sc.n_top(case) == 39 and sc.grid_size(case) == 77 and sc.l_max_of(case) == 77
    assert ms.round_up(sc.n_top(case), k_step) == 40
    n_mu = sc.grid_size(case)
    # three mu blocks of the value form, the last partial; five live blocks of 16 of the Dual form, the last partial
    assert ms.round_up(n_mu, mu_block) // mu_block == 3 and n_mu % mu_block != 0
    assert -(-n_mu // (mu_block // 2)) == 5 and n_mu % (mu_block // 2) != 0
    assert case.nR > 2 * tile_r and case.nR % tile_r != 0           # three radius tiles, the last partial
    assert len(set(case.m)) == len(case.m) and any(m[1] == 0 for m in case.m) and any(m[1] > 0.1 for m in case.m)


def test_tile_k_case_conditions():
    tile_r, _, k_step, _ = ms.kernel_constants()
    case = sc.TILE_K
    n_max = sc.n_max_per_wavelength(case)
    assert case.nR == 8 * tile_r and sc.n_top(case) == 39
    ends, residues, short = [], set(), []
    for row in n_max:
        last = ms.tile_last_n_max(row, tile_r)
        ends.append((int(last[0]), int(last[-1])))
        res, n_short = ms.tile_k_conditions(row, sc.n_top(case), tile_r, k_step)
        residues |= set(res)
        short.append(n_short)
    print(f"tile_k: first and last tile's n_max per wavelength {ends}, residues {sorted(residues)}, tiles ending early {short}")
    assert ends == [(20, 39), (18, 31), (14, 19)]
    assert sorted(residues) == list(range(k_step))
    assert short == [7, 8, 8]


def test_chunk_walk_case_conditions():
    tile_r, mu_block, _, max_chunks = ms.kernel_constants()
    case = sc.CHUNK_WALK
    n_tiles, G, rows, live = ms.chunk_walk_conditions(sc.grid_size(case), case.nR, tile_r, mu_block, max_chunks)
    assert (n_tiles, G, rows, live) == (129, 62, 3, 5)
    n_max = sc.n_max_per_wavelength(case)
    assert sc.n_top(case) <= 14 and int(n_max[1].max()) < int(n_max[0].max())


def test_batch5_case():
    """the repeated wavelengths come with other indices, so no two members of the batch are the same problem"""
    case = sc.BATCH5
    assert len(case.lam) == len(case.m) == 5
    assert len(set(zip(case.lam, case.m))) == 5
    assert case.lam[3] == case.lam[0] and case.lam[4] == case.lam[2] and case.m[3] != case.m[0] and case.m[4] != case.m[2]
    assert case.lam[0] == min(case.lam) and case.lam[-1] == max(case.lam)


def test_spectral_mie_inputs_choose_the_grid_of_the_shortest_wavelength(rtamd):
    S = rtamd.scattering
    aer = S.Aerosol(S.LogNormal(np.log(0.3), np.log(1.6)), 1.3, 0.001)
    lam = np.array([0.55, 0.35, 2.1])
    model = S.make_mie_model(S.NAI2(), aer, 0.55, rtamd.Stokes_IQUV(), S.δBGE(10, 2.0), 1.0, 37)
    inp = S.spectral_mie_inputs(model, lam, autodiff=True)
    single = [S.mie_inputs(S.make_mie_model(S.NAI2(), aer, l, rtamd.Stokes_IQUV(), S.δBGE(10, 2.0), 1.0, 37), True) for l in lam]
    assert [int(v) for v in inp.n_max] == [s.π_.shape[1] for s in single]
    assert inp.n_top == int(S.get_n_max(2 * np.pi / 0.35 * inp.r.max())) == max(int(v) for v in inp.n_max)
    assert inp.μ.size == 2 * inp.n_top - 1 == inp.l_max
    # the shared grid is the single call's own grid at the shortest wavelength; r and w are the single call's at any
    assert np.array_equal(inp.μ, single[1].μ) and np.array_equal(inp.w_μ, single[1].w_μ)
    for s in single:
        assert np.array_equal(inp.r, s.r) and np.array_equal(inp.w, s.w) and inp.w.shape[0] == 3
    assert S.spectral_mie_inputs(model, lam).w.shape[0] == 1


def _stack(pairs, which):
    return {q: np.stack([np.asarray(p[which][q], dtype=np.float64) for p in pairs]) for q in ms.ARRAYS}


def test_checker_tells_the_wavelengths_apart():
    """the oracle's own output passes per wavelength; with two wavelengths exchanged, or with the second a repeat of the first
    (a kernel that ignores the wavelength dimension), it does not"""
    pairs = sc.oracle(sc.BASE)
    good = _stack(pairs, 0)
    assert sc.compare_batch(good, pairs) == []
    swapped = {q: v[[0, 2, 1]] for q, v in good.items()}
    bad = sc.compare_batch(swapped, pairs)
    rows = [v for v in bad if "[" in v[1]]
    print(f"wavelengths 1 and 2 exchanged: {len(bad)} violations, {len(rows)} of them rows")
    assert {j for j, _ in bad} == {1, 2} and len(rows) >= 8
    repeated = {q: v[[0, 0, 2]] for q, v in good.items()}
    bad = sc.compare_batch(repeated, pairs)
    assert bad and {j for j, _ in bad} == {1}


def test_oracle_distances_of_the_base_case():
    """the Float64 / long-double distances that set the bounds of the GPU test, printed; the largest bound stays below 1e-12"""
    for dual in (False, True):
        for j, (o64, o80) in enumerate(sc.oracle(sc.BASE, dual)):
            d = {q: mo.rel_max(np.asarray(o64[q], dtype=np.float64), o80[q]) for q in ms.ARRAYS}
            print(f"{'dual' if dual else 'value'} wavelength {j}: " + ", ".join(f"{q} {v:.1e}" for q, v in d.items()))
            assert all(ms.FACTOR * v < 1e-12 for v in d.values())

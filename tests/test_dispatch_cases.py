"""tests/dispatch_cases.py on the CPU: its restatement of zh_dispatch_kind_dim against a table typed out here, the cells' coverage of all 46
(kind, D) pairs, the rotation's promise over the generic dimensions, and every cell's inputs -- deterministic, and no reference key a NaN.
The 20 tests take 13 s, nearly all of it the 128 cells' key tables (300 calls of the oracle each), 1.1 s for the widest dimension."""
import numpy as np
import pytest

from tests import dispatch_cases as dcs

# metric -> (kind, the dimensions with an instantiation of their own); every other dimension is the generic row loop, D = 0
EVERY = (128, 384, 768)
SIMSIMD = (128, 256, 384, 512, 768, 1024)
LITERAL = {"l2sq": ("K_L2", SIMSIMD), "l2": ("K_L2", SIMSIMD), "cosine": ("K_COS", SIMSIMD), "cosine_corrected": ("K_COS", SIMSIMD),
           "chebyshev": ("K_MAX", EVERY), "canberra": ("K_CANB", EVERY), "bray_curtis": ("K_BRAY", EVERY), "manhattan": ("K_ABS", EVERY),
           "l3": ("K_P3", EVERY), "l4": ("K_P4", EVERY), "hamming": ("K_HAMM", EVERY), "minkowski3": ("K_PP", EVERY), "pnorm65": ("K_PP", EVERY)}
PROBED = (1, 2, 3, 30, 64, 96, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 640, 767, 768, 769, 1023, 1024, 1025, 1500, 1536, 2048)


def test_instantiation_agrees_with_the_literal_table():
    assert set(LITERAL) == set(dcs.NAMES) and len(dcs.NAMES) == 13
    for name, (kind, own) in LITERAL.items():
        for d in PROBED:
            assert dcs.instantiation(name, d) == (kind, d if d in own else 0), (name, d)
    assert len({kind for kind, _ in LITERAL.values()}) == 10 == len(dcs.KINDS)


def test_the_cells_cover_all_46_instantiations():
    every = {(kind, D) for kind, own in LITERAL.values() for D in (0,) + own}
    assert len(every) == 46 and every == dcs.ALL_PAIRS
    assert dcs.coverage(dcs.CELLS) == every
    assert len(dcs.CELLS) == len(set(dcs.CELLS)) == 6 * 13 + 10 * 5
    for d in (128, 256, 384, 512, 768, 1024):
        assert [m for dd, m in dcs.CELLS if dd == d] == list(dcs.NAMES), d  # all thirteen: both L2 forms, both cosine modes, both power forms
    ids = [dcs.cell_id(c) for c in dcs.CELLS]
    assert len(set(ids)) == len(ids) and "d384-canberra" in ids
    assert [d for d, _ in dcs.CELLS] == sorted(d for d, _ in dcs.CELLS)  # dimension by dimension


def test_the_rotation_keeps_its_promise():
    """every generic dimension has L2 squared, parity cosine and three others; every one of the other eleven metrics, and so every kind, meets
    the generic row loop at two of THESE dimensions or more, one of them odd (256 / 512 / 1024 under the eight non-simsimd kinds come on top)"""
    assert dcs.GENERIC == (1, 3, 127, 129, 257, 383, 385, 769, 1025, 1500)
    met = {}
    for d in dcs.GENERIC:
        ms = [m for dd, m in dcs.CELLS if dd == d]
        assert len(ms) == len(set(ms)) == 5 and ms[:2] == ["l2sq", "cosine"], (d, ms)
        for m in ms:
            assert dcs.instantiation(m, d)[1] == 0
            met.setdefault(m, []).append(d)
    assert set(met) == set(dcs.NAMES)
    for m, ds in met.items():
        assert len(ds) >= 2 and any(d % 2 for d in ds), (m, ds)
    by_kind = {}
    for m, ds in met.items():
        by_kind.setdefault(LITERAL[m][0], set()).update(ds)
    assert set(by_kind) == set(dcs.KINDS)
    for kind, ds in by_kind.items():
        assert len(ds) >= 2 and any(d % 2 for d in ds), (kind, ds)
    assert "cosine_corrected" not in [m for d, m in dcs.CELLS if d == 1]  # (two key values there: nothing for the occlusion rule to drop)


def test_the_shared_inputs():
    live = dcs.live_rows()
    live0, live1, g, lines, seeds = dcs.extension()
    assert live.size == 300 and 0 < (~live).sum() < 60
    assert (~live1[dcs.G:]).any(), "some of the 100 appended rows are removed rows"
    assert (~live0[:dcs.G]).any() and (live0[:dcs.G] & ~live1[:dcs.G]).any() and (live1 <= live0).all()
    assert g[0].shape == (dcs.G, dcs.IN_K) and len(lines) == dcs.G and seeds.shape == (dcs.N - dcs.G, dcs.N_SEED)
    assert dcs.X_BATCH < dcs.N - dcs.G and dcs.X_BEAM >= dcs.IN_K
    words, n_bits, mask = dcs.filter_words()
    assert n_bits % 32 and mask.size == n_bits < dcs.N and 0 < (mask & live[:n_bits]).sum() < live[:n_bits].sum()
    ring = dcs.ring()
    assert ring[0].shape == (dcs.N, dcs.IN_K) and (ring[1] == dcs.IN_K).all()


@pytest.mark.parametrize("d", sorted({d for d, _ in dcs.CELLS}))
def test_every_cell_is_deterministic_and_nan_free(d):
    X, live = dcs.table(d)
    Q, seeds = dcs.queries(d)
    assert X.shape == (dcs.N, d) and Q.shape == (dcs.B, d) and seeds.shape == (dcs.B, dcs.N_SEED)
    assert not (X == 0).any() and not (Q == 0).any() and np.isfinite(X).all() and np.isfinite(Q).all()
    first = [a.copy() for a in (X, live, Q, seeds) + dcs.ring() + dcs.extension()[:2] + (dcs.extension()[4],) + dcs.filter_words()[::2]]
    for f in (dcs.table, dcs.queries, dcs.ring, dcs.extension, dcs.filter_words, dcs.live_rows):
        f.cache_clear()
    again = dcs.table(d) + dcs.queries(d) + dcs.ring() + dcs.extension()[:2] + (dcs.extension()[4],) + dcs.filter_words()[::2]
    for a, b in zip(first, again):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    for m in [m for dd, m in dcs.CELLS if dd == d]:
        K, KQ = dcs.keys(d, m)  # (asserts that no key is a NaN)
        om = dcs.METRICS[m][0]
        assert len(K) == dcs.N and KQ.shape == (dcs.B, dcs.N)
        assert not dcs.key_is_nan(np.stack([K[a] for a in range(dcs.N)]), om).any() and not dcs.key_is_nan(KQ, om).any(), (d, m)
        assert len(np.unique(KQ[:, live])) > 8, (d, m)  # (the keys tell rows apart: not one value for all)

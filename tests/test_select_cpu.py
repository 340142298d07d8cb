"""Secure selection without a GPU: the pure-Python model of pack -> mult -> finish gives min, max, argmin and argmax (ties to the
lowest index) for l from 1 to 255, the layout check refuses overflowing widths, and the library exports the selection entries."""
import ctypes
import os
import random
import sys

import pytest

from conftest import oracle_paillier

sys.path.insert(0, os.path.dirname(__file__))
import _select_model as model  # noqa: E402


@pytest.fixture()
def package_layout(monkeypatch):
    """The model run on the package's field layout (SelectLayout offsets, field bits, end) and index width."""
    from protocols.secure_comparison_amd import selection

    own = model.layout

    def layout(kappa, widths, nbits):
        lay = selection.SelectLayout(widths[0], kappa, tuple(widths[1:]), nbits)
        assert (lay.s, lay.offsets, lay.fbits, lay.end) == own(kappa, widths, nbits)
        return lay.s, lay.offsets, lay.fbits, lay.end

    monkeypatch.setattr(model, "layout", layout)
    monkeypatch.setattr(model, "index_bits", selection.index_bits)
    return selection


@pytest.mark.parametrize("l", [1, 16, 32, 64, 255])
def test_model_min_max(keys, l, package_layout):
    sk = oracle_paillier(keys, 1024)
    rng = random.Random(l)
    top = (1 << l) - 1
    pairs = [(0, 0), (0, top), (top, 0), (top, top), (top // 2, top // 2 + (1 if l > 1 else 0))]
    pairs += [(rng.getrandbits(l), rng.getrandbits(l)) for _ in range(4)]
    for x, y in pairs:
        assert model.minimum(sk, x, y, l, rng) == min(x, y)
        assert model.maximum(sk, x, y, l, rng) == max(x, y)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 17])
def test_model_argmin_argmax_ties_to_lowest_index(keys, k, package_layout):
    assert package_layout.tournament_rounds(k) == (k - 1).bit_length() and (1 << package_layout.index_bits(k)) >= k
    sk = oracle_paillier(keys, 1024)
    rng = random.Random(100 + k)
    for l in (1, 16, 255):
        vals = [rng.choice([0, (1 << l) - 1, rng.getrandbits(l)]) for _ in range(k)]
        assert model.argext(sk, vals, l, rng) == (min(vals), vals.index(min(vals)))
        assert model.argext(sk, vals, l, rng, want_max=True) == (max(vals), vals.index(max(vals)))


def test_model_mult_flags_a_foreign_layout(keys, package_layout):
    sk = oracle_paillier(keys, 1024)
    rng = random.Random(3)
    d = model.draw(rng, 40, [64], sk.n)
    P = model.pack(sk, 40, [64], model.enc(sk, 1), [model.enc(sk, (1 << 64) + 5)], d[0], d[1], d[2])
    assert not model.mult(sk, 40, [64], P, d[3])[2]
    assert model.mult(sk, 20, [16], P, d[3])[2]


def test_layout_matches_model_and_rejects_overflow():
    from protocols.secure_comparison_amd.selection import SelectLayout, index_bits

    lay = SelectLayout(255, 40, (index_bits(17),), 1024)
    s, offs, fb, end = model.layout(40, [255, index_bits(17)], 1024)
    assert (lay.s, lay.offsets, lay.fbits, lay.end) == (s, offs, fb, end)
    SelectLayout(255, 40, (), 1024)
    with pytest.raises(ValueError):
        SelectLayout(1000, 40, (), 1024)                     # one product no longer fits
    with pytest.raises(ValueError):
        SelectLayout(450, 40, (450,), 1024)                  # each fits, the packed fields do not
    with pytest.raises(ValueError):
        SelectLayout(32, 0, (), 2048)
    with pytest.raises(ValueError):
        SelectLayout(32, 40, (1, 1, 1, 1), 2048)             # at most four columns
    with pytest.raises(ValueError):
        model.layout(40, [1000], 1024)


def test_library_exports_the_selection_entries():
    from protocols.secure_comparison_amd import _lib
    from protocols.secure_comparison_amd.build import build_lib

    lib = ctypes.CDLL(build_lib(verbose=False))
    for name in ("sc_modexp_var_sq", "sc_select_prep", "sc_select_split"):
        assert hasattr(lib, name)
        assert name in _lib.SYMBOLS
    assert _lib.load().sc_abi_version() == 5

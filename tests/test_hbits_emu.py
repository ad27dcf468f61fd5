"""CPU tier (emulator build of the same kernel sources): the sign-bit words of the hidden activations (dn_block_saved_t.hbits) -- written by
every forward route at C = 64 / 128, read by the chained backward in place of the fp32 activations.  Equalities only; bodies in hbits_cases.py."""
import pytest

import hbits_cases
from test_emu_parity import emu, pytestmark      # noqa: F401  (the emulator-build fixture and its skip condition)


ALL3 = ("seeded", "masks", "none")
TINY = hbits_cases.SIZES[:3]
RAGGED = hbits_cases.SIZES[3]
# The emulator runs a 571-row block call at C = 128 in ~10 s: the three small batches take every combination, the ragged three-mesh batch (several
# workgroups per launch) a few of them; the GPU tier (test_hbits_gpu.py) runs the full cross at every size.
# (waves per workgroup, 16-row halves per wave, dropout modes) per number of meshes
SHAPES = {1: [(0, 1, ALL3), (1, 2, ALL3)], 2: [(1, 1, ALL3), (2, 2, ALL3), (4, 1, ALL3), (4, 2, ALL3), (2, 1, ALL3), (1, 2, ALL3)],
          3: [(2, 1, ("seeded",)), (4, 2, ("masks",))]}


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("sizes", hbits_cases.SIZES)
def test_bits_match_h_on_emulator(emu, sizes, C):
    """case 1, gather form: seeded dropout, explicit masks, no dropout; both MiniMLP depths; waves per workgroup 1, 2, 4 x halves per wave 1, 2"""
    for i, (nw, hh, dropouts) in enumerate(SHAPES[len(sizes)]):
        hbits_cases.run_bits_match_h(emu, sizes, C, 3 if i % 2 == 0 else 2, "gather", nw, hh, dropouts)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("sizes", hbits_cases.SIZES)
def test_bits_match_h_spectral_form_on_emulator(emu, sizes, C):
    """case 1, spectral form (units start at mesh boundaries, not at multiples of 16; one half per wave): every workgroup width"""
    for i, (nw, dropouts) in enumerate({1: [(0, ALL3)], 2: [(1, ALL3), (2, ALL3), (4, ALL3)], 3: [(2, ("seeded",)), (4, ("masks",))]}[len(sizes)]):
        hbits_cases.run_bits_match_h(emu, sizes, C, 3 if i % 2 == 0 else 2, "spectral", nw, 1, dropouts, ran_check=i == 0)


@pytest.mark.parametrize("sizes,C,n_mlp,hh,fallback",
                         [(s, C, n, hh, hh == 1) for s in TINY for C, n in ((128, 3), (64, 2)) for hh in (1, 2)] +
                         [(RAGGED, 64, 2, 1, False), (RAGGED, 64, 3, 2, False)])
def test_backward_from_bits_equals_backward_from_h_on_emulator(emu, sizes, C, n_mlp, hh, fallback):
    """cases 2 and 3: the chained forward's words, and (one wave shape is enough for it) the unfused forward's from the pack kernel, against the
    same saved set with the field NULL"""
    hbits_cases.run_bwd_bits_vs_h(emu, sizes, C, n_mlp, hh, dropout="seeded" if hh == 1 else "masks", fallback=fallback)


def test_shapes_without_a_chained_backward_on_emulator(emu):
    """case 4: C = 256 (no words exist) and n_mlp = 4 (words written, backward unfused)"""
    hbits_cases.run_unchained_backward(emu, (20,), 256, 3, K=32)
    hbits_cases.run_unchained_backward(emu, (20,), 128, 4, K=32)

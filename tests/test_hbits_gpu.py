"""GPU tier: the sign-bit words of the hidden activations (dn_block_saved_t.hbits) on the device -- written by every forward route at
C = 64 / 128, read by the chained backward in place of the fp32 activations.  Equalities only; bodies in hbits_cases.py."""
import pytest

import hbits_cases
from test_gpu_parity import dev      # noqa: F401  (the device fixture)

pytestmark = pytest.mark.gpu

ALL3 = ("seeded", "masks", "none")


@pytest.mark.parametrize("n_mlp", [2, 3])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("sizes", hbits_cases.SIZES)
def test_bits_match_h(dev, sizes, C, n_mlp):
    """case 1, gather form: waves per workgroup 1, 2, 4 x halves per wave 1, 2 (and the default choice), every dropout mode"""
    for nw, hh in [(0, 0)] + [(nw, hh) for nw in (1, 2, 4) for hh in (1, 2)]:
        hbits_cases.run_bits_match_h(dev, sizes, C, n_mlp, "gather", nw, hh, ALL3)


@pytest.mark.parametrize("n_mlp", [2, 3])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("sizes", hbits_cases.SIZES)
def test_bits_match_h_spectral_form(dev, sizes, C, n_mlp):
    """case 1, spectral form (units start at mesh boundaries, not at multiples of 16; one half per wave): every workgroup width"""
    for nw in (0, 1, 2, 4):
        hbits_cases.run_bits_match_h(dev, sizes, C, n_mlp, "spectral", nw, 1, ALL3)


@pytest.mark.parametrize("hh", [1, 2])
@pytest.mark.parametrize("n_mlp", [2, 3])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("sizes", hbits_cases.SIZES)
def test_backward_from_bits_equals_backward_from_h(dev, sizes, C, n_mlp, hh):
    """cases 2 and 3: the chained forward's words and the unfused forward's (pack kernel) against the same saved set with the field NULL"""
    for dropout in ALL3:
        hbits_cases.run_bwd_bits_vs_h(dev, sizes, C, n_mlp, hh, dropout=dropout)


def test_shapes_without_a_chained_backward(dev):
    """case 4: C = 256 (no words exist) and n_mlp = 4 (words written, backward unfused)"""
    hbits_cases.run_unchained_backward(dev, (20,), 256, 3, K=32)
    hbits_cases.run_unchained_backward(dev, (20,), 128, 4, K=32)

"""Host side of TemporalUnet1D at dim = 96 (the reference's `--Unet_dim 96` checkpoint, GroupNorm groups of 12 / 24 / 48 / 96
channels): the handle is created, its manifest is the reference's, synthetic weights load strictly -- no GPU needed.  The widths
that stay refused are refused with the text that names the accepted ones."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O

ACCEPTED_TEXT = "dim must be a power of two >= 32 or 96"


@pytest.mark.parametrize("hz,F,mults,att", [(44, 8, (1, 2, 4, 8), True), (24, 8, (1, 2), False)])
def test_dim96_constructs_and_loads(hz, F, mults, att):
    m = cindm_amd.TemporalUnet1D(hz, F, False, dim=96, dim_mults=mults, attention=att)
    shapes = O.unet1d_param_shapes(hz, F, dim=96, dim_mults=mults, attention=att)
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in shapes.items()}
    synth = O.synth_state_dict(shapes, seed=4)
    m.load_state_dict(synth, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, synth[k]), k


@pytest.mark.parametrize("dim", [48, 80, 160, 192])
def test_other_widths_are_refused_with_the_accepted_set(dim):
    with pytest.raises(cindm_amd.CindmError, match=ACCEPTED_TEXT):
        cindm_amd.TemporalUnet1D(24, 8, False, dim=dim, attention=True)


@pytest.mark.parametrize("dim", [32, 64, 128])
def test_powers_of_two_are_still_accepted(dim):
    assert cindm_amd.TemporalUnet1D(24, 8, False, dim=dim, attention=True).dim == dim

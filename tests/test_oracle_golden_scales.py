"""The CPU oracles at x3, x8 and the wide one-step head against the reference's own outputs (G20, tools/make_golden_scales.py), at the
tolerance tests/test_oracle_golden.py holds their x2 / x4 siblings to."""
import pytest
import torch

import golden_scales as GS


@pytest.mark.parametrize("tag", list(GS.CASES))
def test_g20_oracle_matches_the_reference(tag):
    g, cfg, sd = GS.checked_weights(tag)
    batch = GS.CASES[tag][2]
    for hw in GS.SIZES:
        x = torch.from_numpy(g[f"{tag}.x_{hw[0]}x{hw[1]}"])
        with torch.no_grad():
            y = GS.forward(tag)(sd, cfg, x)
        ref = torch.from_numpy(g[f"{tag}.y_{hw[0]}x{hw[1]}"])
        assert y.shape == ref.shape == (batch, cfg.in_chans, hw[0] * cfg.upscale, hw[1] * cfg.upscale)
        assert (y - ref).abs().max() < 2e-5 * max(1.0, float(ref.abs().max())), (tag, hw)


def test_g20_head_widths_are_the_ones_the_fixture_is_for():
    widths = {tag: GS.config(tag).upscale ** 2 * GS.config(tag).in_chans for tag in ("psd3", "psd4", "psd8g")}
    assert widths == {"psd3": 27, "psd4": 48, "psd8g": 64}

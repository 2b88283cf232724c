"""The command line of --degrade_tables: what the parser accepts, what it refuses, the default, and that the flag leaves no trace in a
checkpoint's saved arguments at its default.  No GPU."""
import pytest

TRAIN = ["--data_root", "D", "--scale", "X2"]
SYNTH = TRAIN + ["--gpu_data", "--synth_lr"]


def test_default_is_host_and_is_not_saved():
    from tpu_superresolution_amd import finetune_swinir as F
    for argv in (TRAIN, SYNTH + ["--degrade", "second_order"], SYNTH + ["--degrade", "blind", "--blur_kernel", "mixed"]):
        a = F.parse_args(argv)
        assert a.degrade_tables == "host" and "degrade_tables" not in F.saved_args(a)


@pytest.mark.parametrize("ok", [
    SYNTH + ["--degrade", "second_order", "--degrade_tables", "device"],
    SYNTH + ["--degrade", "second_order", "--blur_kernel", "mixed", "--degrade_tables", "device"],
    SYNTH + ["--degrade", "blind", "--blur_kernel", "rotated", "--degrade_tables", "device"],
    SYNTH + ["--degrade", "blind", "--blur_kernel", "mixed", "--degrade_tables", "device", "--arch", "hat"],
    SYNTH + ["--degrade", "blind", "--blur_kernel", "mixed", "--degrade_tables", "host"],
    SYNTH + ["--degrade", "blind", "--degrade_tables", "host"],
])
def test_accepted(ok):
    from tpu_superresolution_amd import finetune_swinir as F
    a = F.parse_args(ok)
    assert a.degrade_tables == ok[ok.index("--degrade_tables") + 1]
    assert (F.saved_args(a).get("degrade_tables") == "device") == (a.degrade_tables == "device")


def test_blur_psf_file_goes_with_device_tables(tmp_path):
    import numpy as np
    from tpu_superresolution_amd import blur_kernels as bk, finetune_swinir as F
    f = tmp_path / "psf.npy"
    np.save(f, np.stack([bk.gaussian(7, 1.0, 2.0, 0.3), bk.gaussian(7, 0.8, 0.8)]))
    a = F.parse_args(SYNTH + ["--degrade", "blind", "--blur_psf", str(f), "--degrade_tables", "device"])
    assert a.degrade_tables == "device" and F.psf_spec(a).mode == "file"


@pytest.mark.parametrize("bad", [
    TRAIN + ["--degrade_tables", "device"],                                                   # no degradation at all
    SYNTH + ["--degrade_tables", "device"],                                                   # bicubic has no tables
    SYNTH + ["--degrade", "blind", "--degrade_tables", "device"],                             # the axis-aligned Gaussian has no 2-D table
    SYNTH + ["--degrade", "bicubic", "--degrade_tables", "device"],
    SYNTH + ["--degrade", "second_order", "--degrade_tables", "gpu"],                         # not a choice
    SYNTH + ["--degrade", "second_order", "--degrade_tables"],                                # no value
    TRAIN + ["--task", "dn", "--scale", "X1", "--dn_sigma", "25", "25", "--degrade_tables", "device"],
])
def test_refused(bad, capsys):
    from tpu_superresolution_amd import finetune_swinir as F
    with pytest.raises(SystemExit) as e:
        F.parse_args(bad)
    assert e.value.code == 2 and "error:" in capsys.readouterr().err

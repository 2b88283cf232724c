"""The command-line layer of the data path (data_cli.py) against the record of the parsers it was taken out of.

tests/cli_corpus.json was written by tools/cli_corpus.py --write in a checkout of the commit BEFORE the layer moved (its "recorded_at");
it is not to be regenerated from a later commit.  For every command line of the corpus -- those the host tests of the data path feed to
either parse_args, lines with two faults each, --blur_psf lines -- it holds vars(args), saved_args(args) and the repr of every spec, or
exit code 2 and the text after 'error: '; and the shape of both parsers.  Also here: saved_args by construction, the specs of a run built
once, and the [task] / [synth_lr] / [degrade] lines against those recorded on the device (profiles/cli_refactor_lines.json).  No GPU."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--data_root", "D", "--scale", "X2"]


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CORPUS = _tool("cli_corpus")
with open(os.path.join(ROOT, "tests", "cli_corpus.json")) as _f:
    RECORD = json.load(_f)
ALWAYS = {"data_root", "scale", "weights", "epochs", "batch_size", "lr_patch", "lr", "weight_decay", "workers", "seed", "no_pin", "no_persistent",
          "freeze_regex", "scheduler", "min_lr", "grad_clip", "drop_path_rate", "gpu_data", "gpu_data_shard_mb", "arch", "graph", "freeze_bn",
          "window_size", "augment"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("cli_corpus"))
    CORPUS.write_files(RECORD["files"], root)
    return root


def _json(v):
    return json.loads(json.dumps(v))


def test_the_record_is_the_parents_and_is_whole():
    lines = RECORD["lines"]
    assert RECORD["recorded_at"] == "cb39c42641ea96f7478edbc13f6c3fe5bbe58821"          # the parent commit, clean: no ' (modified)'
    assert (len(lines), sum(not e["ok"] for e in lines), sum(e["ok"] for e in lines)) == (330, 240, 90)
    assert [sum(e["parser"] == w for e in lines) for w in ("finetune", "evaluate")] == [226, 104]
    assert all(e["ok"] or (e["code"] == 2 and e["error"]) for e in lines)
    assert {e["parser"] for e in lines} == {"finetune", "evaluate"}


@pytest.mark.parametrize("i", range(len(RECORD["lines"])))
def test_line(i, files):
    """Entry by entry: an accepted line is accepted with the same vars(args), saved_args and specs, a refused line is refused with the same
    message; and the specs that a run builds at once are those of the nine spec functions."""
    from tpu_superresolution_amd import data_cli
    want = RECORD["lines"][i]
    assert _json(CORPUS.describe(want["parser"], want["argv"], files)) == want
    if not want["ok"]:
        return
    args = CORPUS.modules()[want["parser"]].parse_args([a.replace("@F/", files + os.sep) for a in want["argv"]])
    assert set(vars(args)) == set(CORPUS.defaults(want["parser"]))          # nothing is stored on args
    if want["parser"] == "finetune":
        specs, names = data_cli.train_specs(args), dict(restore="restore_spec", degrade="degrade_spec", second_order="second_order_spec",
                                                        usm="usm_spec", psf="psf_spec", jpeg="jpeg_spec")
        if args.task != "sr":          # the restoration pools code through RestoreSpec: a run has no JpegSpec
            assert specs.jpeg is None
            del names["jpeg"]
    else:
        specs, names = data_cli.eval_specs(args), dict(restore="eval_restore", degrade="degrade", second_order="second_order", usm="eval_usm",
                                                       psf="eval_psf")
    for field, name in names.items():
        assert CORPUS._spec_repr(getattr(specs, field), files) == want["specs"][name], field


@pytest.mark.parametrize("which", ["finetune", "evaluate"])
def test_parser_shape(which):
    """Every action of the parser: option strings, nargs, type, choices, default, metavar, in the order of the parent's."""
    got, want = _json(CORPUS.parser_shape(which)), RECORD["shape"][which]
    assert [a["dest"] for a in got] == [a["dest"] for a in want]
    for a, b in zip(got, want):
        assert a == b, a["dest"]


def test_saved_args_drop_every_later_flag_at_its_default(files):
    from tpu_superresolution_amd import data_cli
    from tpu_superresolution_amd import finetune_swinir as F
    assert set(data_cli.ALWAYS_SAVED) == ALWAYS and set(F.saved_args(F.parse_args(BASE))) == ALWAYS
    ap = F.build_parser()
    later = [a.dest for a in ap._actions if a.dest not in ALWAYS and a.dest != "help"]
    assert len(later) >= 45
    seen = set()
    for e in RECORD["lines"]:          # every accepted training line: a flag it leaves at its default is not saved
        if not (e["ok"] and e["parser"] == "finetune"):
            continue
        args = F.parse_args([a.replace("@F/", files + os.sep) for a in e["argv"]])
        saved = F.saved_args(args)
        for k in later:
            if getattr(args, k) == ap.get_default(k):
                assert k not in saved, (k, e["argv"])
            else:
                seen.add(k)
                owner = data_cli.FOLLOWS.get(k)
                assert (k in saved) == (owner is None or getattr(args, owner) != ap.get_default(owner)), (k, e["argv"])
    assert len(seen) >= 40          # and nearly every one of them is seen off its default, where it is saved


def test_a_flag_added_later_stays_out_of_checkpoints_by_construction():
    from tpu_superresolution_amd import data_cli
    from tpu_superresolution_amd import finetune_swinir as F
    ap = F.build_parser()
    data_cli.flag(ap, "made_up", int, 5, "with --synth_lr: a flag of a later pull request")
    plain, given = ap.parse_args(BASE), ap.parse_args(BASE + ["--made_up", "7"])
    assert plain.made_up == 5 and "made_up" not in data_cli.saved_args(plain, ap)
    assert data_cli.saved_args(given, ap)["made_up"] == 7 and set(data_cli.saved_args(given, ap)) - {"made_up"} == set(data_cli.saved_args(plain, ap))


class _Stub:
    """Stands in for a pool, a data set, a loader or a device wrapper: keeps what it was given."""
    files = ()

    def __init__(self, *a, **kw):
        self.a, self.kw = a, kw

    def __len__(self):
        return 0


def test_psf_file_is_read_once_to_validate_and_once_for_the_run(files, monkeypatch):
    from tpu_superresolution_amd import data_cli, evaluate as E, finetune_swinir as F
    psf, reads, load = os.path.join(files, "own_psf.npy"), [], np.load
    monkeypatch.setattr(np, "load", lambda f, *a, **kw: (reads.append(str(f)), load(f, *a, **kw))[1])
    for name in ("DeviceHRPool", "DeviceHR2Pool", "Shuffled2DHR", "SynthLRBatches", "DevicePoolLoader", "make_loader"):
        monkeypatch.setattr(F, name, _Stub)
    for name in ("Shuffled2DHR", "SynthLRBatches", "DataLoader"):
        monkeypatch.setattr(E, name, _Stub)
    monkeypatch.setattr(F, "train_lines", lambda *a: ["x"])

    for degrade, pool in (("blind", "DeviceHRPool"), ("second_order", "DeviceHR2Pool")):
        del reads[:]
        args = F.parse_args(BASE + ["--gpu_data", "--synth_lr", "--degrade", degrade, "--blur_psf", psf, "--jpeg_quality", "30", "95"])
        assert reads == [psf]
        specs = data_cli.train_specs(args)
        assert reads == [psf] * 2
        train, sampler, valid, lines = F.build_loaders(args, specs, 2, "cpu", 0, 1)
        assert reads == [psf] * 2 and lines == ["x"] and train is sampler
        made = train.a[0]          # the pool inside the DevicePoolLoader, then the validation wrapper: the same instances
        assert made.kw["psf"] is specs.psf is valid.kw["psf"] and valid.kw["degrade"] is specs.degrade and valid.kw["jpeg"] is specs.jpeg
        assert valid.kw["second_order"] is specs.second_order and (specs.second_order is None) == (degrade == "blind")

    del reads[:]
    args = E.parse_args(["--scale", "X2", "--ckpt", "F", "--arch", "swinir", "--synth_lr", "--degrade", "blind", "--blur_psf", psf])
    assert reads == [psf]
    specs = data_cli.eval_specs(args)
    ds, loader = E.build_loader(args, specs, 2, True, torch.device("cpu"))
    assert reads == [psf] * 2 and loader.kw["psf"] is specs.psf and loader.kw["degrade"] is specs.degrade
    assert data_cli.eval_lines(args, specs, 2)[2] == f"[degrade] blur kernel: 5 x 5 table, table 0 of {psf}" and reads == [psf] * 2


def test_weights_envelopes_keep_their_two_orders(tmp_path):
    from tpu_superresolution_amd.evaluate import PARAM_KEYS, _load_state
    f = str(tmp_path / "w.pt")
    torch.save({"params_ema": {"w": torch.tensor(3.0)}, "model": {"w": torch.tensor(1.0)}, "params": {"w": torch.tensor(2.0)}}, f)
    assert PARAM_KEYS == ("model", "params", "params_ema") and float(_load_state(f)[0]["w"]) == 1.0          # evaluate's order
    assert float(_load_state(f, keys=("params", "model", "params_ema"))[0]["w"]) == 2.0          # finetune_swinir --weights
    torch.save({"w": torch.tensor(4.0)}, f)
    assert float(_load_state(f, keys=("params", "model", "params_ema"))[0]["w"]) == 4.0          # a raw state_dict


class _Pool:
    """The numbers of the script tests' data set (tools/cli_lines.py): four 96 x 96 RGB images in one shard; DeviceHR2Pool's window at
    --lr_patch 16, scale 2 and the default margin 8 is (16 + 2 * 8) * 2 = 64 HR pixels."""
    num_shards, extent, margin = 1, 64, 8
    _host = [torch.zeros(4, 96, 96, 3, dtype=torch.uint8)]

    def __len__(self):
        return 4


@pytest.mark.parametrize("run", ["second_order_usm", "blind_psf", "car"])
def test_lines_are_those_recorded_on_the_device(run, files):
    """train_lines / eval_lines, fed a stand-in pool, word the [task] / [synth_lr] / [degrade] lines as the parent printed them."""
    from tpu_superresolution_amd import data_cli, evaluate as E, finetune_swinir as F
    lines_tool = _tool("cli_lines")
    with open(os.path.join(ROOT, "profiles", "cli_refactor_lines.json")) as f:
        parent = json.load(f)["parent"][run]
    with open(os.path.join(files, "psf.npy"), "wb") as f:          # the tables of the tool's data set
        f.write(CORPUS.own_psf_bytes())
    _, scale, train, ev = next(r for r in lines_tool.RUNS if r[0] == run)
    mine = ("[task", "[synth_lr]", "[degrade]", "[gpu_data]")
    args = F.parse_args(lines_tool.train_argv(files, scale, train))
    got = [ln.replace(files, "@W") for ln in data_cli.train_lines(args, data_cli.train_specs(args), data_cli.SCALES[scale], _Pool())]
    assert got == [ln for ln in parent["train_lines"] if ln.startswith(mine)] and len(got) >= 2
    args = E.parse_args(lines_tool.eval_argv(files, files, scale, ev))
    got = [ln.replace(files, "@W") for ln in data_cli.eval_lines(args, data_cli.eval_specs(args), data_cli.SCALES[scale])]
    assert got == [ln for ln in parent["eval_lines"] if ln.startswith(mine)] and len(got) >= 1


def test_second_order_quotes_the_jpeg_range_in_its_own_line():
    """--degrade second_order --jpeg_quality LO HI: the range is the chain's first JPEG's; there is no JpegSpec and no [degrade] jpeg line
    (printing one from the missing spec raised AttributeError on rank 0 before the lines became functions)."""
    from tpu_superresolution_amd import data_cli, finetune_swinir as F
    args = F.parse_args(BASE + ["--gpu_data", "--synth_lr", "--degrade", "second_order", "--jpeg_quality", "40", "90"])
    specs = data_cli.train_specs(args)
    lines = data_cli.train_lines(args, specs, 2, _Pool())
    assert specs.jpeg is None and specs.second_order.jpeg_quality == (40, 90)
    assert [ln[:ln.index(":")] if ":" in ln[:24] else ln[:11] for ln in lines] == ["[synth_lr] ", "[degrade] second order", "[degrade] blind"]
    assert lines[1] == ("[degrade] second order: window 64 x 64 HR px (margin 8 LR px), resize [0.15, 1.5] p=[0.2, 0.7, 0.1] then [0.3, 1.2] "
                        "p=[0.3, 0.4, 0.3], blur 2 p=0.8, sinc p=0.1 final p=0.8, jpeg [40, 90] then [30, 95] chroma 444, seed 0; validation: "
                        "the fixed chain (SecondOrderSpec.fixed), noise id = image index")


def test_tables_are_one_object_in_both_scripts():
    from tpu_superresolution_amd import data_cli, evaluate as E, finetune_swinir as F
    assert F.SCALES is data_cli.SCALES and F.RESTORATION_TASKS is data_cli.RESTORATION_TASKS and E.SCALES is data_cli.SCALES
    assert F.usm_spec is E.eval_usm is data_cli.usm_spec and F.psf_spec is data_cli.psf_spec and E.eval_psf is data_cli.eval_psf
    assert [data_cli.default_window_size(t) for t in ("sr", "dn", "car")] == [8, 8, 7]
    assert types.FunctionType is type(F.saved_args) and F.SECOND_ORDER_FLAGS is data_cli.SECOND_ORDER_FLAGS and F.USM_FLAGS is data_cli.USM_FLAGS

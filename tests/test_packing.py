"""packing.cached_pack / params_version / drop_packs: one cache of packed weights per model with one key rule (pure torch: CPU), and
the import order packing <- host_pass <- hat_arch <- the other architecture files."""
import copy
import os
import re
import subprocess
import sys
import threading

import torch

import tpu_superresolution_amd as T
from tpu_superresolution_amd import dat_train, hat_train, packing, swinir_small_train, swinir_w16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cpu")


def _hat():
    return T.HAT(upscale=2, in_chans=3, img_size=32, window_size=16, compress_ratio=3, squeeze_factor=6, conv_scale=0.01, overlap_ratio=0.5,
                 img_range=1.0, depths=[2, 2], embed_dim=24, num_heads=[2, 2], mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")


def _dat():
    return T.DAT(img_size=32, in_chans=3, embed_dim=48, split_size=[8, 32], depth=[3, 2], num_heads=[4, 4], expansion_factor=2.0, upscale=2,
                 img_range=1.0)


def _swinir():
    return T.SwinIR(img_size=28, in_chans=3, embed_dim=24, depths=(2, 2), num_heads=(2, 2), window_size=7, mlp_ratio=2, img_range=1.0, upscale=2,
                    upsampler="pixelshuffle")


# the seven slots: {slot: packer(model)} per architecture
SLOTS = {
    _hat: {"fwd": lambda m: m._pack(DEV), "T": lambda m: hat_train.pack_transposed(m, DEV)},
    _dat: {"infer": lambda m: m._pack(DEV), "train": lambda m: m._pack(DEV, True), "T": lambda m: dat_train.pack_train(m, DEV)},
    _swinir: {"w16": lambda m: swinir_w16.pack(m, DEV), "wsT": lambda m: swinir_small_train.pack_transposed(m, DEV)},
}


def _pack_all(m, slots):
    return {slot: fn(m) for slot, fn in slots.items()}


def _same_values(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _some_parameters(m):
    ps = list(m.parameters())
    return [ps[0], ps[len(ps) // 2], ps[-1]]


def test_second_call_returns_the_same_dict_and_the_slots_are_the_named_ones():
    torch.manual_seed(0)
    assert sum(len(s) for s in SLOTS.values()) == 7
    for make, slots in SLOTS.items():
        m = make()
        first = _pack_all(m, slots)
        again = _pack_all(m, slots)
        assert all(again[s] is first[s] for s in slots), make.__name__
        assert set(m.__dict__["_packs"]) == set(slots)
        assert len({id(p) for p in first.values()}) == len(slots)          # one dict per slot


def test_a_written_parameter_rebuilds_every_slot_of_its_model_only():
    torch.manual_seed(0)
    for make, slots in SLOTS.items():
        m, other = make(), make()
        kept = _pack_all(other, slots)
        n = len(_some_parameters(m))
        for i in range(n):
            for bump in ("add_", "increment_version"):
                before = _pack_all(m, slots)
                p = _some_parameters(m)[i]
                if bump == "add_":
                    with torch.no_grad():
                        p.add_(0)
                else:
                    torch._C._increment_version([p])
                after = _pack_all(m, slots)
                for s in slots:
                    assert after[s] is not before[s], (make.__name__, s, i, bump)
                    _same_values(after[s], before[s])
                assert all(_pack_all(m, slots)[s] is after[s] for s in slots)
        assert all(_pack_all(other, slots)[s] is kept[s] for s in slots), make.__name__
        assert packing.params_version(m) == 2 * n + packing.params_version(other)


def test_drop_packs_rebuilds_everything():
    torch.manual_seed(0)
    for make, slots in SLOTS.items():
        m = make()
        before = _pack_all(m, slots)
        packing.drop_packs(m)
        assert "_packs" not in m.__dict__
        after = _pack_all(m, slots)
        for s in slots:
            assert after[s] is not before[s]
            _same_values(after[s], before[s])
        packing.drop_packs(m)
        packing.drop_packs(m)                                            # nothing to drop: no error


def test_dat_training_packs_do_not_depend_on_the_buffers():
    """Every training forward bumps num_batches_tracked and moves the running statistics: the `train` and `T` packs read neither, the
    `infer` pack folds the running statistics."""
    torch.manual_seed(0)
    m = _dat()
    slots = SLOTS[_dat]
    first = _pack_all(m, slots)
    bn = m.layers[0].blocks[0].attn.dwconv[1]
    assert isinstance(bn, torch.nn.BatchNorm2d)
    bn.num_batches_tracked += 1
    second = _pack_all(m, slots)
    assert second["train"] is first["train"] and second["T"] is first["T"]
    assert second["infer"] is not first["infer"]
    _same_values(second["infer"], first["infer"])
    bn.running_mean.add_(0.5)
    third = _pack_all(m, slots)
    assert third["train"] is first["train"] and third["T"] is first["T"]
    assert third["infer"] is not second["infer"]
    assert not torch.equal(third["infer"]["0.0.dw_t"], second["infer"]["0.0.dw_t"])


def test_packs_stay_out_of_the_state_dict():
    torch.manual_seed(0)
    for make, slots in SLOTS.items():
        m = make()
        keys = list(m.state_dict().keys())
        _pack_all(m, slots)
        sd = m.state_dict()
        assert list(sd.keys()) == keys and len(sd) == len(keys)
        assert not any("_packs" in k for k in sd)
        fresh = make()
        fresh.load_state_dict(sd, strict=True)
        _same_values(_pack_all(fresh, slots)[next(iter(slots))], _pack_all(m, slots)[next(iter(slots))])


def test_deepcopy_of_a_packed_model():
    torch.manual_seed(0)
    for make, slots in SLOTS.items():
        m = make()
        mine = _pack_all(m, slots)
        c = copy.deepcopy(m)
        with torch.no_grad():
            next(c.parameters()).add_(1.0)
        theirs = _pack_all(c, slots)
        assert all(theirs[s] is not mine[s] for s in slots)
        assert all(_pack_all(m, slots)[s] is mine[s] for s in slots)      # the original's packs are untouched
        fresh = make()
        fresh.load_state_dict(c.state_dict(), strict=True)
        for s in slots:
            _same_values(theirs[s], _pack_all(fresh, slots)[s])           # and the copy's are built from the copy's parameters


def test_two_threads_pack_two_models_at_once():
    torch.manual_seed(0)
    models = [(_hat(), SLOTS[_hat]), (_dat(), SLOTS[_dat])]
    want = [{s: dict(p) for s, p in _pack_all(m, slots).items()} for m, slots in models]
    for m, _ in models:
        packing.drop_packs(m)
    start = threading.Barrier(2)
    got, errors = [None, None], []

    def work(i):
        try:
            m, slots = models[i]
            start.wait(timeout=30)
            for _ in range(3):
                packing.drop_packs(m)
                got[i] = _pack_all(m, slots)
        except Exception as e:          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    for g, w in zip(got, want):
        for s in w:
            assert not any(isinstance(v, packing._Pending) for v in g[s].values())
            assert all(isinstance(v, torch.Tensor) for v in g[s].values())
            _same_values(g[s], w[s])
    assert packing._active() is None


def test_host_pass_imports_on_its_own_and_hat_arch_imports_it_at_the_top():
    r = subprocess.run([sys.executable, "-c", "import tpu_superresolution_amd.host_pass as h, tpu_superresolution_amd.packing as p; "
                        "assert h._rup is p._rup and callable(h._gemm)"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pkg = os.path.join(ROOT, "tpu_superresolution_amd")
    src = {n: open(os.path.join(pkg, n + ".py")).read() for n in ("packing", "host_pass", "hat_arch")}
    assert not re.search(r"^[ \t]+(from|import)\b.*\bhost_pass\b", src["hat_arch"], re.M)          # no function-level import
    assert re.search(r"^from \. import .*\bhost_pass\b", src["hat_arch"], re.M)
    for lower in ("packing", "host_pass"):                                                         # nothing below imports upwards
        assert not re.search(r"^\s*(from|import)\b.*\b(hat_arch|dat_arch|hat_train|dat_train|swinir_w16)\b", src[lower], re.M), lower
    assert not re.search(r"^\s*(from|import)\b.*\bhost_pass\b", src["packing"], re.M)

"""Training with window sizes 2..7: the small-window attention backward kernel (csrc/attn_small_bwd.hip) against autograd on the fp32
restatement of tests/test_gpu_window_small.py and the refusals of its C entry point; whole models (swinir_small_train.py, opted in with
SwinIR.enable_small_window_training) against the reference's G19 gradients and the CPU oracle's autograd; optimizer and graph steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from guarded import Guarded
from oracle import swinir_oracle as O
from test_gpu_window_small import attention_reference
from test_oracle_golden_wsmall import WSMALL, wsmall_weights

pytestmark = pytest.mark.gpu


def _lib():
    from tpu_superresolution_amd import _lib as M
    return M.check, M.lib()


def _case(ws, nH, dh, shift, B, H, W):
    """bf16-rounded inputs of one kernel case and autograd's gradients of the fp32 restatement on them"""
    CA, T = nH * 32, B * H * W
    gen = torch.Generator().manual_seed(1000 * ws + 10 * nH + shift)
    qkv = torch.randn(T, 3, nH, 32, generator=gen) * 0.8
    qkv[..., dh:] = 0.0                                                               # head_dim zero-padded to 32
    qkv = qkv.reshape(T, 3 * CA).to(torch.bfloat16)
    dout = torch.randn(T, nH, 32, generator=gen) * 0.5
    dout[..., dh:] = 0.0
    dout = dout.reshape(T, CA).to(torch.bfloat16)
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=gen)
    scale = dh ** -0.5
    qr = qkv.float().clone().requires_grad_(True)
    tr = table.clone().requires_grad_(True)
    attention_reference(qr, tr, B, H, W, ws, shift, nH, dh, scale).backward(dout.float())
    return qkv, dout, table, scale, qr.grad, tr.grad


@pytest.mark.parametrize("ws", [2, 3, 4, 5, 6, 7])
def test_small_window_attention_backward_vs_autograd(ws):
    """d q / d k / d v / d table against autograd (same bf16-rounded inputs), bounds of test_win256_attention_backward_vs_autograd.
    d_qkv lives in a guarded buffer with ld > 3 CA that starts as NaN: every element of the window is written and nothing outside it;
    d_table is accumulated; d_out = 0 gives d_qkv = 0 exactly and leaves d_table bit-unchanged."""
    check, L = _lib()
    B, H, W = 2, 3 * ws, 5 * ws
    T = B * H * W
    for nH, dh in ((1, 24), (2, 16), (6, 30)) + (((9, 20),) if ws == 7 else ()):
        CA = nH * 32
        for shift in (0, ws // 2):
            what = f"ws {ws} nH {nH} shift {shift}"
            qkv, dout, table, scale, ref_qkv, ref_tab = _case(ws, nH, dh, shift, B, H, W)
            q_d, o_d, t_d = qkv.cuda(), dout.cuda(), table.cuda()
            # d_qkv shares qkv's leading dimension: both get ld = 3 CA + 8; d_qkv starts as NaN with guard rows around it
            dq = Guarded("bf16", T, 3 * CA, 3 * CA + 8)
            dtab = torch.full(((2 * ws - 1) ** 2, nH), 0.75, device="cuda")
            scratch = torch.empty(max(16, int(L.srk_win_small_attention_bwd_scratch(B, H, W, ws, nH))), dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            q_ld = torch.zeros(T, 3 * CA + 8, dtype=torch.bfloat16, device="cuda")
            q_ld[:, :3 * CA] = q_d
            check(L.srk_win_small_attention_bwd(q_ld.data_ptr(), 3 * CA + 8, CA, t_d.data_ptr(), o_d.data_ptr(), CA, dq.ptr, dtab.data_ptr(),
                                                scratch.data_ptr(), B, H, W, ws, shift, nH, scale, st))
            torch.cuda.synchronize()
            dq.assert_guards(what)
            got = dq.data().float()
            assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} elements of d_qkv were not written"
            got, ref = got.view(T, 3, nH, 32), ref_qkv.view(T, 3, nH, 32)
            for i, name in enumerate("qkv"):
                err, big = float((got[:, i] - ref[:, i]).abs().max()), float(ref[:, i].abs().max())
                print(f"{what}: d{name} max err {err:.3e} vs max|ref| {big:.3e}")
                assert err <= 2.5e-2 * big, f"{what}: d{name} max err {err:.3e} vs max|ref| {big:.3e}"
            assert float(got[..., dh:].abs().max()) == 0.0, what
            err_t, big_t = float((dtab.cpu() - 0.75 - ref_tab).abs().max()), float(ref_tab.abs().max())
            print(f"{what}: d table max err {err_t:.3e} vs max|ref| {big_t:.3e}")
            assert err_t <= 2e-2 * max(1.0, big_t), f"{what}: d table (accumulated onto 0.75) max err {err_t:.3e} vs {big_t:.3e}"
            # d_out = 0
            dq0 = Guarded("bf16", T, 3 * CA, 3 * CA + 8)
            before = dtab.clone()
            check(L.srk_win_small_attention_bwd(q_ld.data_ptr(), 3 * CA + 8, CA, t_d.data_ptr(), torch.zeros_like(o_d).data_ptr(), CA, dq0.ptr,
                                                dtab.data_ptr(), scratch.data_ptr(), B, H, W, ws, shift, nH, scale, st))
            torch.cuda.synchronize()
            dq0.assert_guards(what + " (d_out = 0)")
            assert float(dq0.data().float().abs().max()) == 0.0, f"{what}: d_out = 0 must give d_qkv = 0 exactly"
            assert torch.equal(dtab.view(torch.int32), before.view(torch.int32)), f"{what}: d_out = 0 must leave d_table bit-unchanged"


def test_small_window_attention_backward_with_spare_column_blocks():
    """CA = 32 (nH + 1): the column block of q, k and v that holds no head is written as zeros (the coverage rule of d_qkv holds for all
    3 CA columns), the heads' gradients are those of the CA = 32 nH case."""
    check, L = _lib()
    ws, nH, dh, shift, B, H, W = 5, 2, 16, 2, 2, 10, 15
    T, CA0, CA = B * H * W, nH * 32, (nH + 1) * 32
    qkv, dout, table, scale, ref_qkv, ref_tab = _case(ws, nH, dh, shift, B, H, W)
    q_wide = torch.zeros(T, 3, CA, dtype=torch.bfloat16)
    q_wide[:, :, :CA0] = qkv.view(T, 3, CA0)
    q_wide[:, :, CA0:] = 1.0                     # what sits in the spare block must not matter
    dq = Guarded("bf16", T, 3 * CA, 3 * CA + 8)
    q_ld = torch.zeros(T, 3 * CA + 8, dtype=torch.bfloat16, device="cuda")
    q_ld[:, :3 * CA] = q_wide.view(T, 3 * CA).cuda()
    dtab = torch.zeros((2 * ws - 1) ** 2, nH, device="cuda")
    scratch = torch.empty(max(16, int(L.srk_win_small_attention_bwd_scratch(B, H, W, ws, nH))), dtype=torch.uint8, device="cuda")
    t_d, o_d = table.cuda(), dout.cuda()
    check(L.srk_win_small_attention_bwd(q_ld.data_ptr(), 3 * CA + 8, CA, t_d.data_ptr(), o_d.data_ptr(), CA0, dq.ptr,
                                        dtab.data_ptr(), scratch.data_ptr(), B, H, W, ws, shift, nH, scale, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    dq.assert_guards("CA = 32 (nH + 1)")
    got = dq.data().float().view(T, 3, CA)
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} elements of d_qkv were not written"
    assert float(got[:, :, CA0:].abs().max()) == 0.0
    ref = ref_qkv.view(T, 3, CA0)
    for i, name in enumerate("qkv"):
        err, big = float((got[:, i, :CA0] - ref[:, i]).abs().max()), float(ref[:, i].abs().max())
        assert err <= 2.5e-2 * big, f"d{name} max err {err:.3e} vs max|ref| {big:.3e}"
    assert float((dtab.cpu() - ref_tab).abs().max()) <= 2e-2 * max(1.0, float(ref_tab.abs().max()))


def test_small_window_attention_backward_ops_wrapper():
    """ops.window_attention_small_bwd: allocates d_qkv / a zeroed d_table, or accumulates into the d_table it is given"""
    from tpu_superresolution_amd import ops
    ws, nH, dh, shift, B, H, W = 7, 2, 16, 3, 1, 14, 7
    qkv, dout, table, scale, ref_qkv, ref_tab = _case(ws, nH, dh, shift, B, H, W)
    d_qkv, d_tab = ops.window_attention_small_bwd(qkv.cuda(), table.cuda(), dout.cuda(), B, H, W, ws, shift, nH, scale)
    assert d_qkv.shape == qkv.shape and d_qkv.dtype == torch.bfloat16
    assert float((d_qkv.cpu().float() - ref_qkv).abs().max()) <= 2.5e-2 * float(ref_qkv.abs().max())
    assert float((d_tab.cpu() - ref_tab).abs().max()) <= 2e-2 * max(1.0, float(ref_tab.abs().max()))
    _, again = ops.window_attention_small_bwd(qkv.cuda(), table.cuda(), dout.cuda(), B, H, W, ws, shift, nH, scale, d_table=d_tab.clone())
    assert float((again.cpu() - 2 * d_tab.cpu()).abs().max()) <= 1e-5 * max(1.0, float(ref_tab.abs().max()))
    with pytest.raises(ValueError):
        ops.window_attention_small_bwd(qkv.cuda(), table.cuda()[:-1], dout.cuda(), B, H, W, ws, shift, nH, scale)


def test_small_window_attention_backward_refusals():
    check, L = _lib()
    nH, CA = 2, 64
    T = 2 * 14 * 14
    qkv = torch.zeros(T, 3 * CA, dtype=torch.bfloat16, device="cuda")
    dout = torch.zeros(T, CA, dtype=torch.bfloat16, device="cuda")
    dqkv = Guarded("bf16", T, 3 * CA, 3 * CA)
    table = torch.zeros(13 * 13, nH, device="cuda")
    dtab = torch.zeros(13 * 13, nH, device="cuda")
    scratch = torch.empty(int(L.srk_win_small_attention_bwd_scratch(2, 14, 14, 7, nH)), dtype=torch.uint8, device="cuda")
    assert scratch.numel() >= 2 * 4 * nH * 169 * 4
    assert L.srk_win_small_attention_bwd_scratch(2, 16, 16, 8, nH) == 0

    def call(ws, H, W, shift=0, d_qkv=dqkv.ptr, scr=scratch.data_ptr()):
        return L.srk_win_small_attention_bwd(qkv.data_ptr(), 3 * CA, CA, table.data_ptr(), dout.data_ptr(), CA, d_qkv, dtab.data_ptr(), scr, 2, H,
                                             W, ws, shift, nH, 0.25, torch.cuda.current_stream().cuda_stream)
    assert call(8, 16, 8) == -3 and b"2..7" in L.srk_last_error()                        # SRK_E_UNSUPPORTED
    assert call(1, 14, 14) == -3 and b"2..7" in L.srk_last_error()
    assert call(7, 14, 13) == -1 and b"multiple" in L.srk_last_error()                    # SRK_E_SHAPE
    assert call(7, 14, 14, shift=7) == -1 and b"shift_size" in L.srk_last_error()
    assert call(7, 14, 14, d_qkv=None) == -2 and b"null" in L.srk_last_error()            # SRK_E_NULL
    assert call(7, 14, 14, scr=None) == -2 and b"scratch" in L.srk_last_error()
    assert call(7, 14, 14, d_qkv=dqkv.ptr + 2) == -5 and b"aligned" in L.srk_last_error()    # SRK_E_ALIGN
    torch.cuda.synchronize()
    dqkv.assert_untouched("d_qkv of a refused call")
    assert float(dtab.abs().max()) == 0.0


# ---- whole models ---------------------------------------------------------------------------------------------------------------------
def g19_batch(g, cfg):
    h, w = (int(v) for v in g["hw"])
    x = torch.rand(2, cfg.in_chans, h, w, generator=torch.Generator().manual_seed(int(g["x_seed"])))
    t = torch.rand(2, cfg.in_chans, h * cfg.upscale, w * cfg.upscale, generator=torch.Generator().manual_seed(int(g["t_seed"])))
    return x, t


def enabled_model(cfg, sd, drop_path_rate=0.0):
    import tpu_superresolution_amd as T
    m = T.SwinIR(drop_path_rate=drop_path_rate, **cfg.kwargs())
    m.load_state_dict(sd, strict=True)
    return m.cuda().train().enable_small_window_training()


def g19_check(tag, second_backward=True):
    """loss within 2e-3, every gradient tensor within 0.1 relative L2 (median 0.04), every gradient norm within 10 % of the reference's
    (bounds of test_hat_tiny_gradients_vs_reference_golden); -> the measured figures"""
    g19 = load_golden("g19_swinir_wsmall_train")
    _, cfg, sd = wsmall_weights(tag)
    assert str(g19[f"{tag}.weight_sha1"]) == str(load_golden("g17_swinir_wsmall")[f"{tag}.weight_sha1"])
    m = enabled_model(cfg, sd)
    x, t = g19_batch(g19, cfg)
    loss = torch.nn.functional.l1_loss(m(x.cuda()), t.cuda())
    loss.backward()
    ref_loss = float(g19[f"{tag}.loss"])
    print(f"{tag}: loss {float(loss.detach()):.6f} vs reference {ref_loss:.6f}")
    assert abs(float(loss.detach()) - ref_loss) <= 2e-3 * ref_loss
    rels = {}
    names = [n for n, _ in m.named_parameters()]
    assert names == O.param_keys(cfg)
    for n, p in m.named_parameters():
        ref = torch.from_numpy(g19[f"{tag}.grad.{n}"])
        assert p.grad is not None and p.grad.shape == ref.shape, n
        assert torch.isfinite(p.grad).all(), n
        rels[n] = float((p.grad.cpu() - ref).norm() / (ref.norm() + 1e-12))
    worst = max(rels, key=rels.get)
    print(f"{tag}: worst relative L2 gradient error {rels[worst]:.3e} at {worst}, median {float(np.median(list(rels.values()))):.3e}")
    for n, rel in rels.items():
        assert rel <= 0.1, f"{tag} {n}: relative L2 error {rel:.3e}"
    assert float(np.median(list(rels.values()))) <= 0.04
    params = dict(m.named_parameters())
    for n, ref in zip(names, g19[f"{tag}.grad_norms"]):
        got = float(params[n].grad.norm())
        assert abs(got - float(ref)) <= 0.1 * float(ref) + 1e-7, f"{tag} {n}: |grad| {got:.4e} vs reference {float(ref):.4e}"
    if second_backward:      # accumulation semantics: a second backward doubles the gradients
        g1 = {n: p.grad.clone() for n, p in m.named_parameters()}
        torch.nn.functional.l1_loss(m(x.cuda()), t.cuda()).backward()
        for n, p in m.named_parameters():
            assert torch.allclose(p.grad, 2 * g1[n], rtol=2e-3, atol=2e-6 * float(g1[n].abs().max()) + 1e-9), n
    return dict(loss=float(loss.detach()), worst=rels[worst], worst_name=worst)


@pytest.mark.parametrize("tag", sorted(WSMALL))
def test_small_window_tiny_gradients_vs_reference_golden(tag):
    """G19: the reference's training record of the four tiny G17 models on a 2 x C x 16 x 19 batch (reflect padding: T = 882 tokens at
    window 7 -- not a multiple of 64 -- and 640 at window 4), drop_path 0."""
    g19_check(tag)


def test_small_window_gradients_with_poisoned_buffers():
    """The 'ps' tag of G19 in a fresh process with SRK_DBG_POISON=1 (buffers that a kernel must write in full start as NaN): all
    gradients finite and within the same bounds."""
    code = ("import sys, json; sys.path[:0] = %r; import test_gpu_window_small_train as M; "
            "print('RESULT ' + json.dumps(M.g19_check('ps', second_backward=False)))") % ([os.path.dirname(os.path.abspath(__file__)),
                                                                                            os.path.dirname(os.path.dirname(os.path.abspath(__file__)))],)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SRK_DBG_POISON="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert np.isfinite(res["loss"]) and res["worst"] <= 0.1


def _width180_vs_oracle(cfg, B, size, drop_keep):
    """metric of test_hat_width_180_train_step_vs_oracle_autograd: output 2e-2 max|ref|, loss 5e-3, worst gradient error
    |d| / max(|ref|, 2e-3 biggest) <= 0.1 over every parameter"""
    sd = O.random_state_dict(cfg, seed=7, scale=1.0)
    m = enabled_model(cfg, sd, drop_path_rate=0.0 if drop_keep is None else 0.1)
    gen = torch.Generator().manual_seed(4)
    x = torch.rand(B, cfg.in_chans, size, size, generator=gen)
    t = torch.rand(B, cfg.in_chans, size * cfg.upscale, size * cfg.upscale, generator=gen)
    if drop_keep is not None:
        m._drop_override = drop_keep.cuda()
    y = m(x.cuda())
    loss = torch.nn.functional.l1_loss(y, t.cuda())
    loss.backward()
    lo, yo, grads = O.loss_and_grads(sd, cfg, x, t, drop_keep)
    err_y = float((y.detach().cpu() - yo).abs().max())
    print(f"output max err {err_y:.3e} (|ref| max {float(yo.abs().max()):.3f}); loss {float(loss.detach()):.6f} vs {float(lo):.6f}")
    assert err_y <= 2e-2 * float(yo.abs().max())
    assert abs(float(loss.detach()) - float(lo)) <= 5e-3 * float(lo)
    biggest = max(float(g.norm()) for g in grads.values())
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        e = float((p.grad.cpu().float() - grads[n]).norm()) / max(float(grads[n].norm()), 2e-3 * biggest)
        if e > worst[1]:
            worst = (n, e)
    print(f"worst gradient error {worst[1]:.3e} at {worst[0]}")
    assert worst[1] <= 0.1, worst


W180_CAR = dict(upscale=1, in_chans=1, img_size=49, window_size=7, img_range=255.0, depths=(2,), embed_dim=180, num_heads=(6,), mlp_ratio=2,
                upsampler="", resi_connection="1conv")


def test_small_window_width_180_denoise_head_padded_rows_vs_oracle_autograd():
    """embed 180 / 6 heads at window 7, '' head (in_chans 1, img_range 255), B = 8 at 49 x 49: T = 19 208 = 8 (mod 64), so the streaming
    GEMMs run over TR = 19 264 rows with 56 padding rows.  DropPath factors with zeros (the last sample of the last block among them)
    against the oracle given the same factors.  H W = 2401 is no multiple of 64, so with a DropPath factor the MLP runs as the GEMM pair in
    the forward (a 64-row tile of the fused kernel must lie inside one sample) and as the three separate kernels in the backward.  The
    bias, gamma and beta gradients are the ones that would show padding rows left non-zero."""
    cfg = O.SwinIRConfig(**W180_CAR)
    keep = 0.8
    mask = (torch.rand(2, 2, 8, generator=torch.Generator().manual_seed(11)) < keep).float()
    mask[1, :, 7] = 0.0          # the last sample of the last block is dropped in both branches
    mask[0, 0, 0] = 0.0
    _width180_vs_oracle(cfg, 8, 49, mask / keep)


def test_small_window_width_180_fused_mlp_forward_over_padded_rows_vs_oracle_autograd():
    """The same model and batch without DropPath (what a drop_path_rate = 0 fine-tune runs): srk_mlp_fused_fwd_train is launched over
    TR = 19 264 > T = 19 208 rows; the backward's MLP half runs as separate kernels (H W = 2401)."""
    _width180_vs_oracle(O.SwinIRConfig(**W180_CAR), 8, 49, None)


def test_small_window_width_180_fused_mlp_kernels_with_drop_path_vs_oracle_autograd():
    """'pixelshuffledirect' x2, B = 6 at 56 x 56: H W = 49 * 64, so both fused MLP kernels take the DropPath factor (the forward's
    rowscale, the backward's scaled bf16 copy), with zeros among the factors."""
    cfg = O.SwinIRConfig(upscale=2, in_chans=3, img_size=56, window_size=7, img_range=1.0, depths=(2,), embed_dim=180, num_heads=(6,),
                         mlp_ratio=2, upsampler="pixelshuffledirect", resi_connection="1conv")
    keep = 0.75
    mask = (torch.rand(2, 2, 6, generator=torch.Generator().manual_seed(12)) < keep).float()
    mask[1, 1, 5] = 0.0
    mask[0, 0, 2] = 0.0
    _width180_vs_oracle(cfg, 6, 56, mask / keep)


def test_small_window_width_180_pixelshuffle_fused_backward_vs_oracle_autograd():
    """'pixelshuffle' x2, B = 6 at 56 x 56: T = 18 816 = 294 * 64 and H W = 49 * 64, so srk_mlp_fused_bwd and the qkv dgrad with the
    LayerNorm-backward epilogue run; no DropPath."""
    cfg = O.SwinIRConfig(upscale=2, in_chans=3, img_size=56, window_size=7, img_range=1.0, depths=(2,), embed_dim=180, num_heads=(6,),
                         mlp_ratio=2, upsampler="pixelshuffle", resi_connection="1conv")
    _width180_vs_oracle(cfg, 6, 56, None)


# ---- steps ---------------------------------------------------------------------------------------------------------------------------
def test_small_window_fused_adamw_steps_learn_and_ema_moves():
    """Train mode with the default drop_path_rate (0.1) under FusedAdamW (multi-tensor path: the model was enabled first): the loss goes
    down, the weights stay finite, params_ema moves."""
    from tpu_superresolution_amd.optim import FusedAdamW
    _, cfg, sd = wsmall_weights("ps")
    m = enabled_model(cfg, sd, drop_path_rate=0.1)
    opt = FusedAdamW(m, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0, ema_decay=0.9)
    assert opt._flat is False
    torch.manual_seed(0)
    x, t = torch.rand(2, 3, 16, 19, device="cuda"), torch.rand(2, 3, 32, 38, device="cuda")
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.l1_loss(m(x), t)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(torch.isfinite(p).all() for p in m.parameters())
    ema = opt.ema_state_dict()
    key = "layers.0.residual_group.blocks.1.attn.relative_position_bias_table"
    assert not torch.equal(ema[key], sd[key]) and not torch.equal(ema[key], m.state_dict()[key].cpu())


def test_small_window_graphed_train_step_matches_eager_steps():
    """training.GraphedTrainStep on an enabled model: losses of four replayed steps on changing batches against the same steps launched
    eagerly (drop_path 0), bound of the HAT graph test."""
    from tpu_superresolution_amd.training import GraphedTrainStep, l1_loss_checked
    _, cfg, sd = wsmall_weights("ps")
    gen = torch.Generator().manual_seed(9)
    batches = [(torch.rand(2, 3, 16, 19, generator=gen).cuda(), torch.rand(2, 3, 32, 38, generator=gen).cuda()) for _ in range(4)]
    ma, mb = enabled_model(cfg, sd), enabled_model(cfg, sd)
    oa = torch.optim.AdamW(ma.parameters(), lr=1e-4, weight_decay=0.0)
    ob = torch.optim.AdamW(mb.parameters(), lr=1e-4, weight_decay=0.0, capturable=True)
    gs = GraphedTrainStep(mb, ob, max_grad_norm=1.0, warmup=1)

    def eager(x, t):
        oa.zero_grad(set_to_none=True)
        loss, _ = l1_loss_checked(ma(x), t)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ma.parameters(), 1.0)
        oa.step()
        return float(loss.detach())
    eager(*batches[0])                   # the graphed stepper warms up with one eager step on its first batch
    la, lb = [], []
    for x, t in batches:
        la.append(eager(x, t))
        lg, bad = gs(x, t)
        lb.append(float(lg))
        assert int(bad) == 0
    print("eager", la, "graphed", lb)
    assert all(abs(a - b) <= 2e-3 * abs(a) for a, b in zip(la, lb))
    gs.close()


def test_small_window_graphed_step_with_fused_adamw_draws_fresh_drop_path():
    """GraphedTrainStep accepts the enabled model with FusedAdamW; with drop_path > 0 two replays draw different DropPath factors."""
    from tpu_superresolution_amd.optim import FusedAdamW
    from tpu_superresolution_amd.training import GraphedTrainStep
    _, cfg, sd = wsmall_weights("ps")
    m = enabled_model(cfg, sd, drop_path_rate=0.4)
    gs = GraphedTrainStep(m, FusedAdamW(m, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0), warmup=1)
    torch.manual_seed(3)
    x, t = torch.rand(2, 3, 16, 19, device="cuda"), torch.rand(2, 3, 32, 38, device="cuda")
    seen, losses = [], []
    for _ in range(6):
        loss, bad = gs(x, t)
        seen.append(gs.drop.clone())
        losses.append(float(loss))
        assert int(bad) == 0
    assert gs.drop is not None and m._drop_override is gs.drop
    assert any(not torch.equal(seen[i], seen[i + 1]) for i in range(5)) and any(float(v.min()) == 0.0 for v in seen)
    assert all(np.isfinite(losses)) and min(losses[3:]) < losses[0], losses
    gs.close()
    assert m._drop_override is None


# ---- surface -------------------------------------------------------------------------------------------------------------------------
def test_small_window_enabled_model_infers_as_before_and_plain_model_still_refuses():
    import tpu_superresolution_amd as T
    from tpu_superresolution_amd._lib import SrkUnsupported
    _, cfg, sd = wsmall_weights("car")
    x = torch.rand(2, 1, 16, 19, generator=torch.Generator().manual_seed(1)).cuda()

    def plain():
        m = T.SwinIR(**cfg.kwargs())
        m.load_state_dict(sd, strict=True)
        return m.cuda()
    a, b = plain(), plain()
    assert b.enable_small_window_training() is b
    with torch.no_grad():
        assert torch.equal(a.train()(x), b.train()(x))               # train mode under no_grad is inference
    assert torch.equal(a.eval()(x).detach(), b.eval()(x).detach())   # eval mode, grad enabled
    with pytest.raises(SrkUnsupported, match="inference-only"):
        a.train()(x)
    y = b.train()(x)
    assert y.requires_grad and y.shape == (2, 1, 16, 19)


def test_small_window_backward_feeds_the_gradient_hook_once_per_parameter():
    """a stub grad_sync (the interface of distributed.ListGradSynchronizer) sees every parameter's gradient exactly once across its
    segment_done calls, and finish is called"""
    _, cfg, sd = wsmall_weights("psd")
    m = enabled_model(cfg, sd)

    class Stub:
        def __init__(self):
            self.segments, self.finished = [], 0

        def segment_done(self, tensors):
            assert self.finished == 0
            self.segments.append([t.data_ptr() for t in tensors])

        def finish(self):
            self.finished += 1
    m.grad_sync = stub = Stub()
    x, t = torch.rand(2, 3, 16, 19, device="cuda"), torch.rand(2, 3, 32, 38, device="cuda")
    torch.nn.functional.l1_loss(m(x), t).backward()
    n_params = len(list(m.parameters()))
    handed = [p for seg in stub.segments for p in seg]
    assert stub.finished == 1 and len(stub.segments) == 2 + len(cfg.depths)          # tail, every RSTB, head
    assert len(handed) == n_params and len(set(handed)) == n_params
    assert all(p.grad is not None for p in m.parameters())

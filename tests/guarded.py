"""Guarded output buffers of the direct kernel tests (tests/test_gpu_gemm_ex.py, tests/test_gpu_wgrad.py)."""
import torch

GUARD = 256
PAT = {"f32": (torch.int32, 0x7FC0BEEF), "bf16": (torch.int16, 0x7FC1)}       # quiet NaNs with a payload
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


class Guarded:
    """An output buffer [rows][ld] whose data window is [rows][cols], with GUARD rows of NaN pattern before and after it."""

    def __init__(self, kind, rows, cols, ld, fill=None):
        ity, pat = PAT[kind]
        self.kind, self.rows, self.cols, self.ld = kind, rows, cols, ld
        self.raw = torch.full(((rows + 2 * GUARD) * ld,), pat, dtype=ity, device="cuda")
        self.win = self.raw.view(DT[kind])[GUARD * ld:(GUARD + rows) * ld].view(rows, ld)
        if fill is not None:
            self.win[:, :cols] = fill.to(DT[kind]).cuda()
        self.before = self.raw.clone()

    @property
    def ptr(self):
        return self.win.data_ptr()

    def data(self):
        return self.win[:, :self.cols].cpu()

    def assert_guards(self, what):
        keep = torch.ones((self.rows + 2 * GUARD, self.ld), dtype=torch.bool, device="cuda")
        keep[GUARD:GUARD + self.rows, :self.cols] = False
        bad = (self.raw.view(-1, self.ld) != self.before.view(-1, self.ld)) & keep
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the output window were written, first at row/col " \
                                    f"{[int(v) for v in bad.nonzero()[0]]} (window rows {GUARD}..{GUARD + self.rows}, cols 0..{self.cols})"

    def assert_untouched(self, what):
        assert torch.equal(self.raw, self.before), f"{what} was written"

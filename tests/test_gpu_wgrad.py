"""Direct parity of the weight-gradient family (include/srk.h: srk_linear_wgrad_bf16, srk_linear_wgrad_multi_bf16, srk_conv3x3_wgrad_bf16,
srk_conv3x3_wgrad_ps_bf16, srk_img_grad_prep, srk_smallconv_wgrad, srk_smallconv_dgrad, srk_stem_wgrad) through the C ABI against the fp64
restatement in tests/wgrad_ref.py.

Every case runs under each of its option sets (wgrad_ref.option_sets: the kernel-selection switches and a registered / missing / too small
workspace) and checks
  1. values: the exact class with torch.equal (integer operands: every summation order gives the same fp32 bits, so ALL option sets of an
     exact case agree bit for bit), the random / dyadic classes with the DERIVED bound of wgrad_ref.tolerance -- the log line carries
     max(err / tol) per output;
  2. that nothing else is written: 256 guard rows before and after every output keep their NaN payload, bit for bit;
  3. that nothing else is read: the operands sit in buffers with NaN rows before row 0 and after row M, and (ldy > N, ldx > K) NaN in
     the columns outside the slice -- a masked over-read would show as NaN in the result;
  4. the accumulate contract (dW0 / db0 are non-zero; a second call adds the same increment again) and that db == NULL leaves no trace;
  5. the return code.

The comparator's ability to fail and the restated dispatch are pinned on the CPU (tests/test_wgrad_ref.py)."""
import ctypes as C

import pytest
import torch

import wgrad_ref as R
from guarded import Guarded

pytestmark = pytest.mark.gpu

NAN_ROWS = 72            # NaN rows in front of and after every operand (more than one 64-row chunk)
OPTIONS = tuple(R.DEFAULTS)


@pytest.fixture(scope="module")
def L():
    from tpu_superresolution_amd import _lib
    _lib.claim_device(0)
    torch.cuda.set_device(0)
    return _lib


@pytest.fixture(scope="module")
def workspace(L):
    assert int(L.lib().srk_wgrad_workspace_bytes()) == R.WS_FULL
    return torch.empty(R.WS_FULL, dtype=torch.uint8, device="cuda")


def get_option(L, name):
    v = C.c_int()
    L.check(L.lib().srk_get_option(name.encode(), C.byref(v)))
    return v.value


class Operand:
    """A device operand [rows][cols] held as a column slice of a NaN-filled buffer with NaN rows around it."""

    def __init__(self, t2d, ld=0, off=0, pad_rows=NAN_ROWS):
        rows, cols = t2d.shape
        ld = ld or cols
        self.buf = R.embed(t2d, ld, off, before=pad_rows, after=pad_rows).cuda()
        self.ld, self.off, self.pad = ld, off, pad_rows

    def ptr(self, off=None):
        return self.buf.data_ptr() + (self.pad * self.ld + (self.off if off is None else off)) * self.buf.element_size()

    def place(self, t2d, off):
        """A second slice of the same buffer (qkv-style)."""
        self.buf[self.pad:self.pad + t2d.shape[0], off:off + t2d.shape[1]] = t2d.cuda()


def upload(c, inp):
    """The case's operands on the device, once for all its option sets."""
    dev = {}
    if c.kind == "linear":
        shared = {}
        for i, p in enumerate(c.probs):
            if p.ybuf >= 0 and p.ybuf in shared:
                shared[p.ybuf].place(inp[f"y{i}"], p.yoff)
                dev[f"y{i}"] = (shared[p.ybuf], p.yoff)
            else:
                op = Operand(inp[f"y{i}"], p.LDY, p.yoff)
                dev[f"y{i}"] = (op, p.yoff)
                if p.ybuf >= 0:
                    shared[p.ybuf] = op
            dev[f"x{i}"] = (Operand(inp[f"x{i}"], p.LDX, p.xoff), p.xoff)
        return dev
    B, H, W = c.geo
    halo = W + 8                                                   # more NaN pixels than a halo row reaches
    for k, v in inp.items():
        if k.endswith("_0"):
            continue
        if k == "weight":
            dev[k] = Operand(v.reshape(1, -1), pad_rows=1)
        elif k == "d_pred":
            dev[k] = Operand(v.reshape(1, -1), pad_rows=1)
        else:
            dev[k] = Operand(v.reshape(-1, v.shape[-1]), pad_rows=max(NAN_ROWS, halo * c.r * c.r))
    return dev


def outputs(c, inp, prefill=True):
    """name -> Guarded buffer, pre-filled with dW0 / db0."""
    bufs = {}
    f = lambda k: inp[k] if prefill else None
    if c.kind == "linear":
        for i, p in enumerate(c.probs):
            bufs[f"dw{i}"] = Guarded("f32", p.N, p.K, p.K, f(f"dw{i}_0"))
            bufs[f"db{i}"] = Guarded("f32", 1, p.N, p.N, f(f"db{i}_0")[None] if p.db else None)
    elif c.kind in ("conv", "convps"):
        bufs["dw"] = Guarded("f32", c.N, 9 * c.CinP, 9 * c.CinP, f("dw_0"))
        bufs["db"] = Guarded("f32", 1, c.N, c.N, f("db_0")[None] if c.db else None)
    elif c.kind == "imgprep":
        bufs["gy"] = Guarded("f32", c.M, c.CoP, c.CoP)
    elif c.kind == "smalld":
        bufs["dx"] = Guarded("bf16", c.M, c.CinP, c.CinP)
    else:
        n = c.Co * c.Cin * 9
        bufs["dw"] = Guarded("f32", 1, n, n, f("dw_0").reshape(1, n))
        bufs["db"] = Guarded("f32", 1, c.Co, c.Co, f("db_0")[None])
    return bufs


def call(L, c, dev, bufs, no_db=False):
    """One call of the case's entry point -> return code."""
    h = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    if c.kind == "linear":
        db = lambda i, p: bufs[f"db{i}"].ptr if (p.db and not no_db) else None
        if not c.multi:
            p = c.probs[0]
            assert not (p.ldy or p.ldx)
            return h.srk_linear_wgrad_bf16(dev["y0"][0].ptr(), dev["x0"][0].ptr(), bufs["dw0"].ptr, db(0, p), c.M, p.N, p.K, st)
        arr = (L.WgradProblem * len(c.probs))()
        for i, p in enumerate(c.probs):
            (yo, yoff), (xo, xoff) = dev[f"y{i}"], dev[f"x{i}"]
            arr[i].y, arr[i].ldy, arr[i].x, arr[i].ldx = yo.ptr(yoff), p.ldy, xo.ptr(xoff), p.ldx
            arr[i].dw, arr[i].db, arr[i].N, arr[i].K = bufs[f"dw{i}"].ptr, db(i, p), p.N, p.K
        return h.srk_linear_wgrad_multi_bf16(arr, len(c.probs), c.M, st)
    B, H, W = c.geo
    if c.kind in ("conv", "convps"):
        db = bufs["db"].ptr if (c.db and not no_db) else None
        if c.kind == "conv":
            return h.srk_conv3x3_wgrad_bf16(dev["y"].ptr(), dev["x"].ptr(), bufs["dw"].ptr, db, B, H, W, c.CinP, c.N, st)
        return h.srk_conv3x3_wgrad_ps_bf16(dev["y"].ptr(), dev["x"].ptr(), bufs["dw"].ptr, db, B, H, W, c.CinP, c.N, c.r, c.Cs, st)
    if c.kind == "imgprep":
        Hc, Wc = c.img_hw
        inv = R.EXACT_INV_RANGE if c.cls == "exact" else R.IMG_INV_RANGE
        return h.srk_img_grad_prep(dev["d_pred"].ptr(), bufs["gy"].ptr, B, c.Cimg, Hc, Wc, H, W, c.r, c.CoP, inv, st)
    if c.kind == "smallw":
        return h.srk_smallconv_wgrad(dev["x"].ptr(), dev["gy"].ptr(), bufs["dw"].ptr, bufs["db"].ptr, B, H, W, c.Cin, c.CinP, c.Co, c.CoP, st)
    if c.kind == "smalld":
        return h.srk_smallconv_dgrad(dev["gy"].ptr(), dev["weight"].ptr(), bufs["dx"].ptr, B, H, W, c.Cin, c.CinP, c.Co, c.CoP, st)
    return h.srk_stem_wgrad(dev["img4"].ptr(), dev["gy"].ptr(), bufs["dw"].ptr, bufs["db"].ptr, B, H, W, c.Cin, c.Co, c.CoP, st)


def run(L, workspace, c, inp, dev, opts, ws_bytes, repeat=1, no_db=False):
    """`repeat` calls under the option set on fresh guarded outputs -> {name: Guarded}.  Options and the workspace registration are
    restored on every way out."""
    h = L.lib()
    was = {k: get_option(L, k) for k in OPTIONS}
    bufs = outputs(c, inp)
    try:
        for k in OPTIONS:
            L.check(h.srk_set_option(k.encode(), opts.get(k, R.DEFAULTS[k])))
        L.check(h.srk_set_wgrad_workspace(workspace.data_ptr() if ws_bytes else None, ws_bytes))
        for _ in range(repeat):
            rc = call(L, c, dev, bufs, no_db)
            assert rc == 0, (rc, h.srk_last_error().decode())
        torch.cuda.synchronize()
    finally:
        for k, v in was.items():
            L.check(h.srk_set_option(k.encode(), v))
        L.check(h.srk_set_wgrad_workspace(None, 0))
    return bufs


def read(c, bufs, exp):
    """The outputs the reference names, shaped like the reference."""
    return {k: bufs[k].data().reshape(o.ref.shape) for k, o in exp.items()}


def twice(exp, inp):
    """The expectation after a second call on the same outputs (accumulating kinds): old + 2 * increment."""
    return {k: R.Out(2 * o.ref - inp[k + "_0"].double(), 2 * o.tol, o.kind) for k, o in exp.items()}


_cache = {}


def prepared(c):
    if c.id not in _cache:
        _cache.clear()                                   # the large references and device operands: keep one case
        inp = R.make_inputs(c)
        _cache[c.id] = (inp, R.expected(c, inp), upload(c, inp))
    return _cache[c.id]


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_values_guards_and_contracts(L, workspace, c):
    inp, exp, dev = prepared(c)
    sets = R.option_sets(c)
    got, worst, kernels = {}, {k: 0.0 for k in exp}, set()
    for name, (opts, ws) in sets.items():
        bufs = run(L, workspace, c, inp, dev, opts, ws)
        for k, b in bufs.items():
            b.assert_guards(f"{c.id} [{name}] {k}")
            if k not in exp:
                b.assert_untouched(f"{c.id} [{name}] {k} (db == NULL)")
        got[name] = read(c, bufs, exp)
        ok, ratios = R.accepts(c, got[name], exp)
        assert ok, f"[{name}] kernels {R.EXPECTED_KERNEL(c, opts, ws)}: max(err / tol) {ratios}"
        worst = {k: max(worst[k], v) for k, v in ratios.items()}
        kernels.update(R.EXPECTED_KERNEL(c, opts, ws))
    first = next(iter(sets))
    if c.cls == "exact" or c.kind == "imgprep":
        for name in sets:                                # integer sums: every kernel, split and summation order gives the same bits
            for k in exp:
                assert torch.equal(bits(got[name][k]), bits(got[first][k])), (name, k)
    elif c.kind == "linear" and "ring32-ws" in sets:
        # the contracts the header states: w8 = 0 / 1 sum in the same order; with partials the order is fixed, so a repeat gives the
        # same dW (db goes through fp32 atomics in every variant)
        for a, b in (("ring32-ws", "ring32_w4-ws"), ("ring64-ws", "ring64_w4-ws")):
            for k in exp:
                if k.startswith("dw"):
                    assert torch.equal(bits(got[a][k]), bits(got[b][k])), (a, b, k)
        again = read(c, run(L, workspace, c, inp, dev, *sets["ring32-ws"]), exp)
        for k in exp:
            if k.startswith("dw"):
                assert torch.equal(bits(again[k]), bits(got["ring32-ws"][k])), k
    elif c.kind in ("conv", "convps", "stem") and "ws" in first:
        again = read(c, run(L, workspace, c, inp, dev, *sets[first]), exp)
        repeatable = R.EXPECTED_KERNEL(c, *sets[first])[-1].split("<")[0].endswith("reduce_kernel")
        if repeatable:                                   # split partials summed in a fixed order
            assert torch.equal(bits(again["dw"]), bits(got[first]["dw"]))
    # the accumulate contract: a second call adds the same increment again
    if c.kind in R.ACCUMULATING:
        opts, ws = sets[first]
        bufs = run(L, workspace, c, inp, dev, opts, ws, repeat=2)
        for k, b in bufs.items():
            b.assert_guards(f"{c.id} twice {k}")
        ok, ratios = R.accepts(c, read(c, bufs, exp), twice(exp, inp))
        assert ok, f"second call: {ratios}"
    # db == NULL leaves no trace (the entry points whose db is optional)
    if c.kind in ("linear", "conv", "convps") and any(R.has_db(c, i) for i in range(max(1, len(c.probs)))):
        opts, ws = sets[first]
        bufs = run(L, workspace, c, inp, dev, opts, ws, no_db=True)
        for k, b in bufs.items():
            if k.startswith("db"):
                b.assert_untouched(f"{c.id} {k} with db == NULL")
            else:
                b.assert_guards(f"{c.id} {k} with db == NULL")
        dw_only = {k: o for k, o in exp.items() if k.startswith("dw")}
        ok, ratios = R.accepts(c, read(c, bufs, dw_only), dw_only)
        assert ok, f"db == NULL: {ratios}"
    print(f"[wgrad] {c.id} sets={len(sets)} kernels={sorted(kernels)} " + " ".join(f"{k}:{v:.3f}" for k, v in worst.items()))


def test_pad_channels_of_dx_are_zero_bits(L, workspace):
    """srk_smallconv_dgrad writes all CinP columns; the ones >= Cin are +0."""
    for c in R.CASES:
        if c.kind == "smalld" and c.Cin < c.CinP and c.cls == "exact":
            inp, exp, dev = prepared(c)
            for name, (opts, ws) in R.option_sets(c).items():
                dx = run(L, workspace, c, inp, dev, opts, ws)["dx"].data()
                assert bool((bits(dx[:, c.Cin:]) == 0).all()), (c.id, name)

"""
The case tables of the native optimizer step (mzx_optim_step, csrc/mzx_optim.h), shared by tests/test_native_optim.py
(the serial build) and tests/test_gpu_native_optim.py (the device): flat lengths, span tables, values, hyperparameter
rows, the numpy float32 restatement of the definition in include/mzx.h, and the checks both builds have to pass.  The
entry is called through ctypes on plain tensors; no network is needed.
"""
import ctypes
import itertools

import numpy
import torch

from mzx import _lib

LENGTHS = (1, 63, 64, 65, 255, 257, 1023, 1025, 4099)
NAN_BITS = 0x7FC00123      # what every array holds in a skipped span: a NaN with a payload, compared bit for bit
F32 = numpy.float32


# ---------------------------------------------------------------------------------------------------------------------
# Span tables: lists of (offset, count); what they do not cover is skipped.

def span_tables(n):
    tables = {"whole": [(0, n)]}
    spans, at, live = [], 0, True
    for width in itertools.cycle((1, 2, 3, 5, 7)):      # live 1, skipped 2, live 3, skipped 5, live 7, skipped 1, live 2, ...
        if at >= n:
            break
        width = min(width, n - at)
        if live:
            spans.append((at, width))
        at, live = at + width, not live
    tables["alternating"] = spans                        # nothing 16-byte aligned
    if n >= 3:
        first, last = max(1, n // 5), max(1, n // 7)
        tables["skipped_ends"] = [(first, n - first - last)]      # a skipped span first and one last
    tables["empty_spans"] = [(0, 0), (0, n // 2), (n // 2, 0), (n, 0)]      # the second half is skipped
    tables["reversed"] = [(n - n // 3, n // 3), (0, n // 3)]      # not in offset order; the middle is skipped
    return tables


def live_mask(n, spans):
    mask = numpy.zeros(n, dtype=bool)
    for off, count in spans:
        assert not mask[off:off + count].any()
        mask[off:off + count] = True
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# Values.

def values(n, seed, state):
    """p of both signs, g with magnitudes from 1e-20 to 1e3 (g * g lands in the subnormals and below), exact +0.0 and -0.0
    in both; ``state``: "zero" or "random" (m of both signs, v >= 0 down to the subnormals) -> dict of float32 arrays."""
    rs = numpy.random.RandomState(seed)
    p = rs.standard_normal(n).astype(F32)
    g = (10.0 ** rs.uniform(-20, 3, n) * rs.choice([-1.0, 1.0], n)).astype(F32)
    for k, x in enumerate((0.0, -0.0)):
        p[k + 1::11] = x
        g[k + 3::13] = x
    if state == "zero":
        m, v = numpy.zeros(n, F32), numpy.zeros(n, F32)
    else:
        m = (rs.standard_normal(n) * 10.0 ** rs.uniform(-12, 1, n)).astype(F32)
        v = (10.0 ** rs.uniform(-44, 2, n)).astype(F32)
        m[2::17] = -0.0
        v[4::19] = 0.0
    return dict(p=p, g=g, m=m, v=v)


ADAM = dict(lr=0.02, betas=(0.9, 0.999), eps=1e-8)
ADAM_ROWS = [dict(name=f"t{t}_{state}_wd{wd:g}", t=t, state=state, wd=wd, **ADAM)
             for t, state in ((1, "zero"), (2, "random"), (1000, "random")) for wd in (0.0, 1e-4)]
SGD_ROWS = [dict(name=f"mu{mu:g}_{'first' if first else 'later'}_wd{wd:g}", mu=mu, first=first, wd=wd, lr=0.05,
                 state="zero" if first else "random", t=1 if first else 3)
            for mu, first in ((0.0, True), (0.9, True), (0.9, False)) for wd in (0.0, 1e-4)]


# ---------------------------------------------------------------------------------------------------------------------
# The scalars, in binary64 as torch computes them (torch/optim/adam.py, _single_tensor_adam), and the restatement.

def adam_scalars(row, t=None, lr=None):
    t = row["t"] if t is None else t
    lr = row["lr"] if lr is None else lr
    beta1, beta2 = row["betas"]
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    return dict(weight_decay=row["wd"], one_minus_beta1=1 - beta1, beta2=beta2, one_minus_beta2=1 - beta2, eps=row["eps"],
                step_size=lr / bias_correction1, bias_correction2_sqrt=bias_correction2 ** 0.5)


def adam_restated(p, g, m, v, s):
    """The definition in include/mzx.h, every operation a float32 one -> (p, m, v)."""
    wd, c1, b2, c2 = F32(s["weight_decay"]), F32(s["one_minus_beta1"]), F32(s["beta2"]), F32(s["one_minus_beta2"])
    bc2s, eps, neg_ss = F32(s["bias_correction2_sqrt"]), F32(s["eps"]), F32(-s["step_size"])
    with numpy.errstate(all="ignore"):
        gd = g + wd * p if wd != 0 else g
        m = m + (gd - m) * c1
        v = v * b2 + (c2 * gd) * gd
        den = numpy.sqrt(v) / bc2s + eps
        p = p + neg_ss * (m / den)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


def sgd_restated(p, g, buf, row, lr=None):
    wd, mu, neg_lr = F32(row["wd"]), F32(row["mu"]), F32(-(row["lr"] if lr is None else lr))
    with numpy.errstate(all="ignore"):
        gd = g + wd * p if wd != 0 else g
        if row["mu"] == 0:
            return p + neg_lr * gd, buf
        buf = gd if row["first"] else buf * mu + gd
        p = p + neg_lr * buf
    assert p.dtype == buf.dtype == F32
    return p, buf


# ---------------------------------------------------------------------------------------------------------------------
# The call.

def chunk_table(be, spans, n):
    """(host span array, device chunk table, number of chunks) of a span list (mzx_optim_chunks)."""
    h_spans = numpy.ascontiguousarray(numpy.asarray(spans, dtype=numpy.int64).reshape(-1, 2))
    count = int(be.lib.mzx_optim_chunks(h_spans.ctypes.data, len(h_spans), n, None, 0))
    assert count >= 0, be.lib.mzx_last_error()
    chunks = numpy.zeros((max(count, 1), 2), dtype=numpy.int64)
    assert be.lib.mzx_optim_chunks(h_spans.ctypes.data, len(h_spans), n, chunks.ctypes.data, count) == count
    return h_spans, torch.from_numpy(chunks).to(be.device), count


def optim_io(be, kind, arrays, spans, scalars, keep, t=1, first=False, momentum=0.0, lr=0.0, misaligned=False):
    """A complete mzx_optim_io over device copies of ``arrays`` (p, g, and m / v or buf) -> (io, the device tensors).
    ``misaligned``: every array starts four bytes behind a 16-byte boundary (no 16-byte access is possible)."""
    n = len(arrays["p"])
    d = {k: torch.from_numpy(numpy.array(v, dtype=F32)).to(be.device) for k, v in arrays.items() if v is not None}
    if misaligned:
        for key, tensor in d.items():
            base = torch.zeros(n + 4, dtype=torch.float32, device=be.device)
            first = next(k for k in range(4) if (base.data_ptr() + 4 * k) % 16 == 4)
            d[key] = base[first:first + n]
            d[key].copy_(tensor)
            assert d[key].data_ptr() % 16 == 4 and d[key].numel() == n
    h_spans, d_chunks, count = chunk_table(be, spans, n)
    keep.append((d, h_spans, d_chunks))
    io = _lib.OptimIO()
    io.kind, io.first_step, io.t, io.n = kind, int(first), t, n
    io.d_param, io.d_grad = d["p"].data_ptr(), d["g"].data_ptr()
    if kind == _lib.OPTIM_ADAM:
        io.d_state1, io.d_state2 = d["m"].data_ptr(), d["v"].data_ptr()
        for key, value in scalars.items():
            setattr(io, key, value)
    else:
        io.d_state1 = d["buf"].data_ptr() if "buf" in d else None
        io.weight_decay, io.lr, io.momentum = scalars["wd"], lr, momentum
    io.h_spans, io.num_spans, io.d_chunks, io.num_chunks = h_spans.ctypes.data, len(h_spans), d_chunks.data_ptr(), count
    return io, d


def sync(be):
    if be.device.type == "cuda":
        torch.cuda.synchronize()


def step(be, io):
    rc = be.lib.mzx_optim_step(ctypes.byref(io), be.stream())
    assert rc == 0, be.lib.mzx_last_error()
    sync(be)


def bits(x):
    return numpy.ascontiguousarray(x).view(numpy.int32)


def poisoned(arrays, mask):
    """Copies with NAN_BITS in every skipped element."""
    out = {}
    for key, x in arrays.items():
        x = x.copy()
        bits(x)[~mask] = NAN_BITS
        out[key] = x
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The checks.

def check_adam_bits(be, n, table, row, seed=0, misaligned=False):
    """One Adam step over one span table equals the restatement bit for bit on the live spans; the skipped spans keep their
    NaN bits in p, g, m and v."""
    spans = span_tables(n)[table]
    mask = live_mask(n, spans)
    start = poisoned(values(n, 1000 * seed + n, row["state"]), mask)
    scalars = adam_scalars(row)
    keep = []
    io, d = optim_io(be, _lib.OPTIM_ADAM, start, spans, scalars, keep, t=row["t"], misaligned=misaligned)
    step(be, io)
    want = dict(zip("pmv", adam_restated(start["p"], start["g"], start["m"], start["v"], scalars)))
    want["g"] = start["g"]
    for key in "pgmv":
        got = d[key].cpu().numpy()
        expect = numpy.where(mask, want[key], start[key])
        bits(expect)[~mask] = NAN_BITS
        assert not numpy.isnan(expect[mask]).any()
        differ = numpy.nonzero(bits(got) != bits(expect))[0]
        assert differ.size == 0, (f"{key}: {differ.size} of {n} elements differ, first at {differ[0]} ({'live' if mask[differ[0]] else 'skipped'}): "
                                  f"{got[differ[0]]!r} for {expect[differ[0]]!r}")


def check_sgd_bits(be, n, table, row, seed=0):
    spans = span_tables(n)[table]
    mask = live_mask(n, spans)
    raw = values(n, 2000 * seed + n, row["state"])
    start = dict(p=raw["p"], g=raw["g"])
    if row["mu"] != 0:
        # the first step never reads the buffer: whatever it holds (here a NaN everywhere) is overwritten on the live spans
        start["buf"] = numpy.full(n, numpy.nan, F32) if row["first"] else raw["m"]
    start = poisoned(start, mask)
    keep = []
    io, d = optim_io(be, _lib.OPTIM_SGD, start, spans, dict(wd=row["wd"]), keep, t=row["t"], first=row["first"],
                     momentum=row["mu"], lr=row["lr"])
    step(be, io)
    p, buf = sgd_restated(start["p"], start["g"], start.get("buf"), row)
    want = dict(p=p, g=start["g"], buf=buf)
    for key in start:
        got = d[key].cpu().numpy()
        expect = numpy.where(mask, want[key], start[key])
        bits(expect)[~mask] = NAN_BITS
        assert not numpy.isnan(expect[mask]).any()
        differ = numpy.nonzero(bits(got) != bits(expect))[0]
        assert differ.size == 0, (f"{key}: {differ.size} of {n} elements differ, first at {differ[0]}: "
                                  f"{got[differ[0]]!r} for {expect[differ[0]]!r}")


def check_nan_gradient(be, kind, n=257, at=70):
    """A NaN gradient lands in that element's parameter and state and nowhere else (its bits are not compared)."""
    spans = span_tables(n)["whole"]
    start = values(n, 7, "random")
    start["g"][at] = numpy.nan
    keep = []
    if kind == "adam":
        row = ADAM_ROWS[3]
        scalars = adam_scalars(row)
        io, d = optim_io(be, _lib.OPTIM_ADAM, start, spans, scalars, keep, t=row["t"])
        want = dict(zip("pmv", adam_restated(start["p"], start["g"], start["m"], start["v"], scalars)))
    else:
        row = SGD_ROWS[5]
        start = dict(p=start["p"], g=start["g"], buf=start["m"])
        io, d = optim_io(be, _lib.OPTIM_SGD, start, spans, dict(wd=row["wd"]), keep, t=row["t"], first=False, momentum=row["mu"],
                         lr=row["lr"])
        want = dict(zip(("p", "buf"), sgd_restated(start["p"], start["g"], start["buf"], row)))
    step(be, io)
    others = numpy.arange(n) != at
    for key, expect in want.items():
        got = d[key].cpu().numpy()
        assert numpy.isnan(got[at]) and numpy.isnan(expect[at]), key
        assert not numpy.isnan(got[others]).any(), key
        assert numpy.array_equal(bits(got)[others], bits(expect)[others]), key


# Against torch: four consecutive steps of torch.optim.Adam / SGD on the CPU in binary64 and in float32 on the same inputs
# (defaults: the single-tensor implementation).  The grid the restatement alone passes on: n = 4099 elements, parameters
# N(0, 1), a fresh gradient per step with magnitudes log-uniform over the six decades 1e-3 .. 1e3 and random signs (with
# Adam's lr = 0.02 every step moves an element by about lr whatever its gradient's size, with SGD's lr = 1e-4 by up to 0.1),
# weight decay 1e-4, SGD momentum 0.9.  The yardstick is torch itself: the largest absolute parameter error of the native
# result against the binary64 run may be at most 4 x that of torch's float32 run.
TORCH_N, TORCH_STEPS, TORCH_GATE = 4099, 4, 4.0
TORCH_HP = {"adam": dict(lr=0.02, weight_decay=1e-4), "sgd": dict(lr=1e-4, momentum=0.9, weight_decay=1e-4)}


def torch_inputs():
    rs = numpy.random.RandomState(99)
    p = rs.standard_normal(TORCH_N).astype(F32)
    grads = [(10.0 ** rs.uniform(-3, 3, TORCH_N) * rs.choice([-1.0, 1.0], TORCH_N)).astype(F32) for _ in range(TORCH_STEPS)]
    return p, grads


def torch_run(kind, dtype):
    p, grads = torch_inputs()
    param = torch.nn.Parameter(torch.from_numpy(p).to(dtype))
    make = torch.optim.Adam if kind == "adam" else torch.optim.SGD
    optimizer = make([param], **TORCH_HP[kind])
    for g in grads:
        param.grad = torch.from_numpy(g).to(dtype)
        optimizer.step()
    return param.detach().to(torch.float64).numpy()


def native_run(be, kind):
    """The same four steps through mzx_optim_step on one set of device arrays."""
    p, grads = torch_inputs()
    hp = TORCH_HP[kind]
    n, keep = TORCH_N, []
    zeros = numpy.zeros(n, F32)
    if kind == "adam":
        row = dict(ADAM, wd=hp["weight_decay"], lr=hp["lr"])
        io, d = optim_io(be, _lib.OPTIM_ADAM, dict(p=p, g=grads[0], m=zeros, v=zeros), [(0, n)], adam_scalars(row, t=1), keep)
    else:
        io, d = optim_io(be, _lib.OPTIM_SGD, dict(p=p, g=grads[0], buf=zeros), [(0, n)], dict(wd=hp["weight_decay"]), keep,
                         first=True, momentum=hp["momentum"], lr=hp["lr"])
    for t, g in enumerate(grads, 1):
        d["g"].copy_(torch.from_numpy(g))
        io.t, io.first_step = t, int(t == 1)
        if kind == "adam":
            for key, value in adam_scalars(row, t=t).items():
                setattr(io, key, value)
        step(be, io)
    return d["p"].cpu().numpy().astype(numpy.float64)


def check_against_torch(be, kind, report=print):
    exact = torch_run(kind, torch.float64)
    theirs = float(numpy.abs(torch_run(kind, torch.float32) - exact).max())
    mine = float(numpy.abs(native_run(be, kind) - exact).max())
    report(f"{kind}: {TORCH_STEPS} steps, n = {TORCH_N}: native error {mine:.3e} against binary64, torch float32's own {theirs:.3e} "
           f"({mine / theirs if theirs else float('inf'):.2f} x; gate {TORCH_GATE:g} x)")
    assert theirs > 0
    assert mine <= TORCH_GATE * theirs


# Every refusal: the io of a good call with one thing wrong -> MZX_ERR_INVALID, an error text, nothing written.
REFUSALS = ["d_param", "d_grad", "d_state1", "d_state2", "h_spans", "d_chunks", "span_below_zero", "span_past_the_end",
            "span_count_negative", "spans_overlap", "t=0", "t=-3", "momentum_without_buffer", "unknown_kind", "num_chunks"]


def check_refusal(be, what, n=257):
    start = {k: numpy.full(n, 7.0, F32) for k in "pgmv"}
    keep = []
    kind = _lib.OPTIM_SGD if what == "momentum_without_buffer" else _lib.OPTIM_ADAM
    if kind == _lib.OPTIM_ADAM:
        io, d = optim_io(be, kind, start, [(0, 100), (100, 57), (200, 57)], adam_scalars(ADAM_ROWS[0]), keep, t=1)
    else:
        io, d = optim_io(be, kind, dict(p=start["p"], g=start["g"]), [(0, n)], dict(wd=0.0), keep, momentum=0.9, lr=0.1, first=True)
    bad = {"span_below_zero": [(-1, 5)], "span_past_the_end": [(n - 3, 4)], "span_count_negative": [(5, -1)],
           "spans_overlap": [(0, 100), (150, 50), (99, 10)]}
    if what in bad:
        h_spans = numpy.asarray(bad[what], dtype=numpy.int64)
        keep.append(h_spans)
        io.h_spans, io.num_spans = h_spans.ctypes.data, len(h_spans)
        assert be.lib.mzx_optim_chunks(h_spans.ctypes.data, len(h_spans), n, None, 0) == -1
    elif what.startswith("t="):
        io.t = int(what[2:])
    elif what == "unknown_kind":
        io.kind = 2
    elif what == "num_chunks":
        io.num_chunks += 1
    elif what != "momentum_without_buffer":
        setattr(io, what, None)
    assert be.lib.mzx_optim_step(ctypes.byref(io), be.stream()) == -1      # MZX_ERR_INVALID
    assert be.lib.mzx_last_error()
    sync(be)
    for key, t in d.items():
        assert (t == 7.0).all(), key

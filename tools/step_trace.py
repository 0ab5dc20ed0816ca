"""What HDPissaStep launches, in order (comparison tool, not part of the library).

  python tools/step_trace.py [--device cpu|cuda] [--summary] [--only SUBSTRING] [--out FILE]
                             [--compute-dtype bfloat16]

Wraps an op set and a communicator in a recording proxy and drives the stepper through a matrix of
configurations -- the three exchanges, world sizes, dtypes, merge roundings, gradient clipping, bucket bounds,
HDP_DELTA_GROUPED, a two-arena model.  Every call on the op set, on the communicator and on the plans that
``delta_plan`` returns is one line: the method and every argument, a tensor as ``buffer+byte_offset:numel:dtype``
with ``buffer`` found by address among the named buffers (W<j>; per arena grad, m, v, delta, fac, fac_all; the
arena plan's exchange buffers; the stepper's clip buffers).  A tensor in no named buffer prints as ``?`` and the
tool exits non-zero.  Each configuration runs: two steps, invalidate_factors(), a step, one W_res moved to new
storage, a step -- so the cache-rebuild paths appear.

The communicator is a single-process stand-in (every simulated rank holds this rank's buffer): the values are
irrelevant, only the calls are recorded.

--device cpu   the op sets of the host tests (CpuOps + the stochastic-rounding and clip test op sets).
--device cuda  HipOps; every line carries the current stream (main / side), and Event.record / Stream.wait_event
               are logged (patched inside this tool only) with the event's index in order of first use.
--compute-dtype bfloat16   another axis, off by default (the default matrix and its bytes stay): the layers keep
               bf16 copies of their float32 W_res (named L<j>) and the trace gains the step's shadow_group calls;
               configuration names end in -cdbfloat16; all-bf16 configurations are left out (nothing to copy).
--summary      one line per configuration: name, line count, SHA-1 of its lines (tests/golden/step_trace_cpu.txt).

Two commits that launch the same things print the same bytes:
  python tools/step_trace.py > a.txt      (in each tree)      diff a.txt b.txt
The tool reads only names the stepper keeps, so the same file runs on either commit.
"""
import argparse
import contextlib
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-pissa_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

CPU_SHAPES = [(48, 40), (20, 40), (64, 24), (40, 56)]          # out = 20 at Wn = 4: a short block, a rank with no rows
GPU_SHAPES = [(256, 192), (128, 192), (200, 320), (384, 250)]  # tests/test_gpu_ranks_shard.py
NAMES = ["q_proj", "k_proj", "o_proj", "up_proj"]
DTYPES = {"f32": [torch.float32] * 4, "bf16": [torch.bfloat16] * 4,
          "mixed": [torch.bfloat16, torch.float32, torch.bfloat16, torch.float32]}
LR = 2e-3


class Recorder:
    """The lines of one configuration and the table of named buffers."""

    def __init__(self):
        self.lines, self.bufs, self.unnamed = [], [], 0
        self.tag = lambda: ""
        self.nplans = 0

    def name(self, name, t):
        if t is not None and t.numel():
            self.bufs.append((name, t.data_ptr(), t.numel() * t.element_size()))

    def tensor(self, t):
        dt = str(t.dtype).replace("torch.", "")
        if not t.numel():
            return "empty:%s" % dt
        p = t.data_ptr()
        for name, base, nbytes in self.bufs:
            if base <= p < base + nbytes:
                return "%s+%d:%d:%s" % (name, p - base, t.numel(), dt)
        self.unnamed += 1
        return "?:%d:%s" % (t.numel(), dt)

    def fmt(self, x):
        if isinstance(x, torch.Tensor):
            return self.tensor(x)
        if isinstance(x, (list, tuple)):
            return "[" + ", ".join(self.fmt(y) for y in x) + "]"
        if isinstance(x, torch.device):
            return str(x)
        return repr(x)

    def log(self, text):
        self.lines.append(self.tag() + text)


class Proxy:
    """Records every method call on ``inner``; attributes that are no methods (and missing ones: hasattr
    answers as the wrapped object does) pass through."""

    def __init__(self, inner, rec, prefix):
        self.__dict__.update(_inner=inner, _rec=rec, _prefix=prefix)

    def __getattr__(self, attr):
        val = getattr(self._inner, attr)
        if not callable(val):
            return val
        rec, prefix = self._rec, self._prefix

        def call(*args, **kw):
            text = "%s.%s(%s)" % (prefix, attr, ", ".join([rec.fmt(a) for a in args] +
                                                          ["%s=%s" % (k, rec.fmt(v)) for k, v in kw.items()]))
            if attr == "delta_plan":
                rec.nplans += 1
                name = "plan%d" % rec.nplans
                rec.log(text + " -> " + name)
                return Proxy(val(*args, **kw), rec, name)
            res = val(*args, **kw)
            if isinstance(res, torch.Tensor):  # (a new allocation: no named buffer yet)
                text += " -> tensor:%d:%s" % (res.numel(), str(res.dtype).replace("torch.", ""))
            elif res is not None:
                text += " -> " + rec.fmt(res)
            rec.log(text)
            return res
        return call


class EchoComm:
    """Single-process stand-in for Wn ranks: every rank holds this rank's buffer."""
    name = "echo"

    def __init__(self, rank, world_size):
        self.rank, self.world_size = rank, world_size

    def allgather(self, send, recv):
        self.allgather_any(send, recv)

    def allgather_any(self, send, recv):
        recv.reshape(-1).view(torch.uint8).view(self.world_size, -1).copy_(send.reshape(-1).view(torch.uint8))

    def allreduce_sum(self, buf):
        buf.mul_(self.world_size)

    def alltoall(self, send, recv):
        recv.view(self.world_size, -1).copy_(send.view(self.world_size, -1)[self.rank])

    def broadcast(self, t, root):
        return None


def cpu_ops(shadow=False):
    from test_clip_host import ClipCpuOps
    from test_sr_host import SrCpuOps

    class TraceCpuOps(ClipCpuOps, SrCpuOps):
        name = "cpu-test-trace"

    class ShadowTraceCpuOps(TraceCpuOps):
        def shadow_group(self, pairs):
            for dst, src in pairs:
                dst.copy_(src)
    return ShadowTraceCpuOps() if shadow else TraceCpuOps()


def grads(L, j, rank, step):
    g = torch.Generator().manual_seed(1000 * step + 10 * j + rank)
    return torch.randn(L.A.shape, generator=g) * 1e-14, torch.randn(L.B.shape, generator=g) * 1e-14


def configs(device, compute_dtype=None):
    """(name, settings) of every configuration of the matrix, in a fixed order."""
    out = []
    if device == "cpu":
        ranks = [(1, 0), (2, 1), (4, 3), (4, 2)]
        for ex, (wn, rank), dts, mr, clip, bb, grouped in itertools.product(
                ("gather", "allreduce", "shard"), ranks, DTYPES, ("nearest", "stochastic"), (None, 1.0),
                (None, 1024), ("1", "0")):
            if mr == "stochastic" and dts == "f32":
                continue
            out.append(dict(exchange=ex, wn=wn, rank=rank, dts=dts, rounding=mr, clip=clip, bucket=bb,
                            grouped=grouped, arenas=1, r=4))
        out.append(dict(exchange="gather", wn=1, rank=0, dts="f32", rounding="nearest", clip=1.0, bucket=None,
                        grouped="1", arenas=2, r=4))
    else:
        for ex in ("gather", "allreduce", "shard"):
            ranks = [(1, 0), (2, 1)] + ([(8, 7)] if ex == "shard" else [])
            for (wn, rank), dts, mr, clip, bb in itertools.product(
                    ranks, DTYPES, ("nearest", "stochastic"), (None, 1.0), (None, 100_000)):
                if mr == "stochastic" and dts == "f32":
                    continue
                # r = 32 with bf16 W: the Wn = 1 fused Adam-pack path (r Wn <= 128 = the smallest dimension)
                r = 16 if dts == "f32" or wn == 8 else 32
                out.append(dict(exchange=ex, wn=wn, rank=rank, dts=dts, rounding=mr, clip=clip, bucket=bb,
                                grouped="1", arenas=1, r=r))
    for c in out:
        c["name"] = "%s-w%dr%d-%s-%s-clip%s-bb%s-g%s-a%d" % (
            c["exchange"], c["wn"], c["rank"], c["dts"], c["rounding"], c["clip"], c["bucket"], c["grouped"], c["arenas"])
        c["compute_dtype"] = None
    if compute_dtype is not None:
        out = [c for c in out if c["dts"] != "bf16"]
        for c in out:
            c["compute_dtype"] = compute_dtype
            c["name"] += "-cd" + compute_dtype
    return out


def name_buffers(rec, st, layers):
    rec.bufs = []
    for j, L in enumerate(layers):
        rec.name("W%d" % j, L.W_res)
        rec.name("L%d" % j, getattr(L, "W_lp", None))
    for k, plan in enumerate(st.plans):
        a, pre = plan.arena, "a%d." % k
        for attr in ("grad", "m", "v", "delta", "fac", "fac_all"):
            rec.name(pre + attr, getattr(a, attr))
        for attr, val in sorted(vars(plan).items()):  # delta_all and both halves of every double buffer
            if isinstance(val, torch.Tensor):
                rec.name(pre + attr, val)
            elif isinstance(val, (list, tuple)) and val and all(isinstance(x, torch.Tensor) for x in val):
                for q, x in enumerate(val):
                    rec.name("%s%s[%d]" % (pre, attr, q), x)
    for attr in ("_sums", "_sums_all", "clip_state"):
        rec.name(attr, getattr(st, attr, None))


def run_config(c, device):
    """The lines of one configuration (and the number of tensors that matched no named buffer)."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    dev = torch.device("cuda:0" if device == "cuda" else "cpu")
    rec = Recorder()
    if device == "cuda":
        from hdpissa_amd.ops import default_ops
        real, shapes = default_ops(), GPU_SHAPES
    else:
        real, shapes = cpu_ops(c["compute_dtype"] is not None), CPU_SHAPES
    model = nn.Module()
    g = torch.Generator().manual_seed(5)
    for name, (out, inn), dt in zip(NAMES, shapes, DTYPES[c["dts"]]):
        lin = nn.Linear(inn, out, bias=False)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
        setattr(model, name, lin.to(dev).to(dt).requires_grad_(False))
    groups = [NAMES] if c["arenas"] == 1 else [NAMES[:2], NAMES[2:]]
    layers = []
    for names in groups:  # (no communicator: every simulated rank decomposes every module itself)
        ckw = {} if c["compute_dtype"] is None else {"compute_dtype": getattr(torch, c["compute_dtype"])}
        layers += replace_with_custom_layer(model, names, c["rank"], c["wn"], c["r"], 16.0, ops=real, **ckw)
    old = os.environ.get("HDP_DELTA_GROUPED")
    os.environ["HDP_DELTA_GROUPED"] = c["grouped"]
    try:
        kw = {} if c["bucket"] is None else {"bucket_bytes": c["bucket"]}
        st = HDPissaStep(model, c["wn"], c["rank"], comm=Proxy(EchoComm(c["rank"], c["wn"]), rec, "comm"),
                         ops=Proxy(real, rec, "ops"), exchange=c["exchange"], max_grad_norm=c["clip"],
                         merge_rounding=c["rounding"], sr_seed=77 if c["rounding"] == "stochastic" else None, **kw)
    finally:
        if old is None:
            os.environ.pop("HDP_DELTA_GROUPED", None)
        else:
            os.environ["HDP_DELTA_GROUPED"] = old
    if device == "cuda":
        rec.tag = lambda: "[side] " if torch.cuda.current_stream(dev) == st.side else "[main] "

    def step(t):
        name_buffers(rec, st, layers)
        for j, L in enumerate(layers):
            gA, gB = grads(L, j, c["rank"], t)
            L.A.grad, L.B.grad = gA.to(dev), gB.to(dev)
        rec.lines.append("# step %d" % t)
        st.step(LR, t)

    with patched_events(rec, st) if device == "cuda" else contextlib.nullcontext():
        step(1)
        step(2)
        rec.lines.append("# invalidate_factors")
        st.invalidate_factors()
        step(3)
        rec.lines.append("# W1 moved")
        layers[1].W_res = layers[1].W_res.clone()
        if getattr(layers[1], "W_lp", None) is not None:
            layers[1].refresh_shadow()  # (a W_res replaced by hand: the caller's refresh)
        step(4)
        if device == "cuda":
            torch.cuda.synchronize()
    return rec.lines, rec.unnamed


@contextlib.contextmanager
def patched_events(rec, st):
    """Log Event.record and Stream.wait_event (an event's number: the order of first use in the configuration)."""
    rec_orig, wait_orig = torch.cuda.Event.record, torch.cuda.Stream.wait_event
    count = itertools.count(1)

    def idx(ev):
        if "_trace_idx" not in ev.__dict__:
            ev.__dict__["_trace_idx"] = next(count)
        return ev.__dict__["_trace_idx"]

    def sname(s):
        return "side" if s == st.side else "main"

    def record(self, stream=None):
        s = torch.cuda.current_stream() if stream is None else stream
        rec.log("event%d.record(%s)" % (idx(self), sname(s)))
        return rec_orig(self, s)

    def wait_event(self, event):
        rec.log("%s.wait_event(event%d)" % (sname(self), idx(event)))
        return wait_orig(self, event)

    torch.cuda.Event.record, torch.cuda.Stream.wait_event = record, wait_event
    try:
        yield
    finally:
        torch.cuda.Event.record, torch.cuda.Stream.wait_event = rec_orig, wait_orig


def run_matrix(device="cpu", only=None, progress=False, compute_dtype=None):
    """[(name, lines, unnamed tensors)] of every configuration (whose name contains ``only``)."""
    out = []
    for c in configs(device, compute_dtype):
        if only and only not in c["name"]:
            continue
        lines, unnamed = run_config(c, device)
        out.append((c["name"], lines, unnamed))
        if progress:
            print("%s: %d lines" % (c["name"], len(lines)), file=sys.stderr, flush=True)
    return out


def summary_line(name, lines):
    return "%s %d %s" % (name, len(lines), hashlib.sha1("\n".join(lines).encode()).hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--only", default=None, help="run the configurations whose name contains this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary-out", default=None, help="also write the --summary form to this file")
    ap.add_argument("--progress", action="store_true", help="name every finished configuration on stderr")
    ap.add_argument("--compute-dtype", default=None, choices=["bfloat16"],
                    help="the matrix again with bf16 compute copies of the float32 modules (names end in -cd<dtype>)")
    args = ap.parse_args()
    if args.device == "cuda" and not torch.cuda.is_available():
        raise SystemExit("--device cuda needs a HIP device")
    res = run_matrix(args.device, args.only, args.progress, args.compute_dtype)
    text = []
    for name, lines, _ in res:
        text += [summary_line(name, lines)] if args.summary else ["## " + name] + lines
    body = "\n".join(text) + "\n"
    if args.summary_out:
        with open(args.summary_out, "w") as f:
            f.write("".join(summary_line(name, lines) + "\n" for name, lines, _ in res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(body)
    else:
        sys.stdout.write(body)
    bad = [(n, u) for n, _, u in res if u]
    if bad:
        raise SystemExit("tensors in no named buffer: " + ", ".join("%s (%d)" % b for b in bad))


if __name__ == "__main__":
    main()

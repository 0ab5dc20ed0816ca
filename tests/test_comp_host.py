"""merge_rounding="compensated" on the host (CPU): the step's logic through a test-only op set (CpuOps + the two
opt-in bf16 merges from their numpy replicas) -- Wn = 1 and gloo Wn = 2 under every exchange against the replica,
every rank and every exchange bitwise equal in W_res and W_c, the constructor's gates, float32 modules of a mixed
model untouched, the state (W_c is no state_dict entry, survives a rebuilt stepper, is zeroed for a layer whose
W_res was written), resume, and the reason for the mode: the drift of 128 small steps."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from cpu_ops import CpuOps, _seg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [("q_proj", 75, 130), ("o_proj", 128, 192)]
R, LR = 16, 2e-3


class CompCpuOps(CpuOps):
    """CpuOps + merge_group_comp and merge_group_sr from the numpy replicas -- TEST ONLY.  K4 is formed one
    rank-1 term at a time with element-wise operations, so that a row block of a module gets the bits the whole
    module gets (a BLAS product gives no such promise): the shard exchange can then be held to the gather
    exchange bit for bit."""
    name = "cpu-test-comp"

    def __init__(self, factors=None):
        super().__init__(factors)
        self.comp_calls = []

    def merge_group_comp(self, triples):
        from hdpissa_amd.rounding import comp_merge_reference
        for W, C, dW in triples:
            assert W.dtype == torch.bfloat16 and C.dtype == torch.bfloat16 and dW.dtype == torch.float32
            assert W.numel() == dW.numel() == C.numel() and W.shape == C.shape
            self.comp_calls.append(W.numel())
            w, c = comp_merge_reference(W, C, dW.reshape(W.shape))
            W.copy_(w)
            C.copy_(c)

    def merge_group_sr(self, triples, seed):
        from hdpissa_amd.rounding import sr_merge_reference
        for W, dW, elem0, offset in triples:
            W.copy_(sr_merge_reference(W, dW.reshape(W.shape), elem0, seed, offset))

    def delta_gemm(self, out, inn, r, nseg, dA, dB, delta_stride, A, B, factor_stride, dst, mode, round_bf16):
        run = torch.zeros(out, inn)
        for i in range(nseg):
            a = _seg(A, i, factor_stride, r * inn, (r, inn))
            b = _seg(B, i, factor_stride, out * r, (out, r))
            da = _seg(dA, i, delta_stride, r * inn, (r, inn))
            db = _seg(dB, i, delta_stride, out * r, (out, r))
            amd = a - da
            term = torch.zeros(out, inn)
            for k in range(r):
                term = term + db[:, k:k + 1] * amd[k:k + 1, :]
                term = term + b[:, k:k + 1] * da[k:k + 1, :]
            run = run - term
            if round_bf16:
                run = run.bfloat16().float()
        d = dst.reshape(-1)[:out * inn].view(out, inn)
        if mode == 0:
            d.copy_(run)
        elif d.dtype == torch.bfloat16:
            d.copy_((d.float() + run.bfloat16().float()).bfloat16())
        else:
            d.add_(run)


def _model(shapes, dts, seed=5):
    model = nn.Module()
    g = torch.Generator().manual_seed(seed)
    for (name, out, inn), dt in zip(shapes, dts):
        lin = nn.Linear(inn, out, bias=False)
        with torch.no_grad():
            lin.weight.copy_((torch.randn(out, inn, generator=g) * 0.05).bfloat16().float())
        setattr(model, name, lin.to(dt).requires_grad_(False))
    return model


def _grads(L, j, rank, step):
    g = torch.Generator().manual_seed(1000 * step + 10 * j + rank)
    return torch.randn(L.A.shape, generator=g) * 1e-14, torch.randn(L.B.shape, generator=g) * 1e-14


def _set_grads(layers, step, rank=0):
    for j, L in enumerate(layers):
        L.A.grad, L.B.grad = _grads(L, j, rank, step)


def _build(dts=(torch.bfloat16, torch.bfloat16), ops=None, **kw):
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    ops = CompCpuOps() if ops is None else ops
    model = _model(SHAPES, dts)
    layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], 0, 1, R, float(R), ops=ops)
    kw.setdefault("merge_rounding", "compensated")
    return model, layers, HDPissaStep(model, 1, 0, ops=ops, **kw), ops


def _bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _store_dw(ops, arena, j, L):
    """The float32 dW of module j on the deltas K3 left in the arena (this rank's segment only)."""
    oa, ob = arena.offsets[j]
    dW = torch.zeros(L.out_features, L.in_features)
    ops.delta_gemm(L.out_features, L.in_features, L.r, 1, arena.delta[oa:], arena.delta[ob:], 0, arena.fac[oa:],
                   arena.fac[ob:], 0, dW, 0, False)
    return dW


# ------------------------------------------------------------------------------------------ Wn = 1
@pytest.mark.parametrize("exchange", ["gather", "allreduce", "shard"])
def test_wn1_equals_replica(exchange):
    from hdpissa_amd.rounding import comp_merge_reference
    _, layers, st, ops = _build(exchange=exchange)
    assert st.plans[0].sr and st.plans[0].comp and st.sr_seed is None
    arena = layers[0]._arena
    for L in layers:
        assert L.W_c is not None and L.W_c.dtype == torch.bfloat16 and L.W_c.shape == L.W_res.shape
        assert not L.W_c.any()
    for step in (1, 2):
        _set_grads(layers, step)
        before = [(L.W_res.clone(), L.W_c.clone()) for L in layers]
        st.step(LR, step)
        for j, L in enumerate(layers):
            w, c = comp_merge_reference(*before[j], _store_dw(ops, arena, j, L))
            assert _same(L.W_res, w) and _same(L.W_c, c), (step, j)
            assert not torch.equal(L.W_res, before[j][0]) and L.W_c.any()
    assert sorted(ops.comp_calls) == sorted([75 * 130, 128 * 192] * 2)


# ------------------------------------------------------------------------------------------ gloo, Wn = 2
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, wn, port, exchange, outdir):
    import sys
    for p in (HERE, ROOT, os.path.join(ROOT, "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from hdpissa_amd.comm import TorchComm
        from hdpissa_amd.rounding import comp_merge_reference
        from test_comp_host import LR, R, SHAPES, CompCpuOps, _grads, _model, _same
        model = _model(SHAPES, [torch.bfloat16] * 2)
        comm, ops = TorchComm(rank, wn), CompCpuOps()
        layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], rank, wn, R, float(R), comm=comm, ops=ops)
        st = HDPissaStep(model, wn, rank, comm=comm, ops=ops, exchange=exchange, bucket_bytes=20000,
                         merge_rounding="compensated")
        arena = layers[0]._arena
        F, fac = arena.F, arena.fac_all.view(-1)
        for step in (1, 2):
            for j, L in enumerate(layers):
                L.A.grad, L.B.grad = _grads(L, j, rank, step)
            before = [(L.W_res.clone(), L.W_c.clone()) for L in layers]
            st.step(LR, step)
            for j, L in enumerate(layers):
                for name, t in (("W_res", L.W_res), ("W_c", L.W_c)):
                    x = t.view(torch.int16).to(torch.int32)  # (gloo has no 16-bit integers)
                    xs = [torch.zeros_like(x) for _ in range(wn)]
                    dist.all_gather(xs, x)
                    assert all(torch.equal(xs[0], y) for y in xs), f"step {step} module {j}: {name} differs across ranks"
                assert not torch.equal(L.W_res, before[j][0]) and L.W_c.any()
            # (W, W_c) = the replica on the pre-step pair and the float32 dW of the same items: the plain float32
            # sum over the ranks' terms, no per-rank bf16 rounding
            deltas = [torch.zeros(F) for _ in range(wn)]
            dist.all_gather(deltas, arena.delta.clone())
            dall = torch.cat(deltas)
            for j, L in enumerate(layers):
                oa, ob = arena.offsets[j]
                dW = torch.zeros(L.out_features, L.in_features)
                if exchange == "allreduce":  # every rank's own term, summed by the collective
                    for k in range(wn):
                        part = torch.zeros_like(dW)
                        ops.delta_gemm(L.out_features, L.in_features, L.r, 1, deltas[k][oa:], deltas[k][ob:], 0,
                                       fac[k * F + oa:], fac[k * F + ob:], 0, part, 0, False)
                        dW += part
                else:  # one K4 over the Wn segments (shard: its row blocks, which have the whole module's bits)
                    ops.delta_gemm(L.out_features, L.in_features, L.r, wn, dall[oa:], dall[ob:], F, fac[oa:], fac[ob:], F,
                                   dW, 0, False)
                w, c = comp_merge_reference(*before[j], dW)
                assert _same(L.W_res, w) and _same(L.W_c, c), (exchange, step, j)
        torch.save([(L.W_res.clone(), L.W_c.clone()) for L in layers], os.path.join(outdir, f"{exchange}_{rank}.pt"))
    except Exception as e:  # surface the assertion text to the parent
        import traceback
        with open(os.path.join(outdir, "err.txt"), "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def gloo_runs(tmp_path_factory):
    """Each exchange once at Wn = 2 (the workers check ranks and replica themselves): exchange -> rank 0's result."""
    out = {}
    for exchange in ("gather", "allreduce", "shard"):
        d = str(tmp_path_factory.mktemp(exchange))
        try:
            mp.spawn(_worker, args=(2, _port(), exchange, d), nprocs=2, join=True)
            out[exchange] = torch.load(os.path.join(d, f"{exchange}_0.pt"))
        except Exception:
            err = os.path.join(d, "err.txt")
            out[exchange] = "worker failed:\n" + (open(err).read() if os.path.exists(err) else "")
    return out


@pytest.mark.parametrize("exchange", ["gather", "allreduce", "shard"])
def test_gloo_ranks_bitwise_equal_and_replica(gloo_runs, exchange):
    assert not isinstance(gloo_runs[exchange], str), gloo_runs[exchange]


def test_gloo_shard_equals_gather_bitwise(gloo_runs):
    g, s = gloo_runs["gather"], gloo_runs["shard"]
    assert not isinstance(g, str) and not isinstance(s, str), (g, s)
    for j, ((gw, gc), (sw, sc)) in enumerate(zip(g, s)):
        assert _same(gw, sw) and _same(gc, sc), j
        assert gc.any()


# ------------------------------------------------------------------------------------------ gates, mixed model
def test_gates():
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    model = _model(SHAPES[:1], [torch.bfloat16])
    ops = CpuOps()
    assert not hasattr(ops, "merge_group_comp")
    (L,) = replace_with_custom_layer(model, ["q_proj"], 0, 1, 4, 16.0, ops=ops)
    with pytest.raises(NotImplementedError):
        HDPissaStep(model, 1, 0, ops=ops, merge_rounding="compensated")
    assert L.W_c is None
    HDPissaStep(model, 1, 0, ops=ops)  # "nearest" needs nothing new
    with pytest.raises(ValueError):
        HDPissaStep(model, 1, 0, ops=CompCpuOps(), merge_rounding="up")
    assert L.W_c is None


@pytest.mark.parametrize("exchange", ["gather", "allreduce"])
def test_mixed_model_float32_module_untouched(exchange):
    from hdpissa_amd.rounding import comp_merge_reference
    runs = {}
    for mode in ("nearest", "compensated"):
        _, layers, st, ops = _build((torch.float32, torch.bfloat16), exchange=exchange, merge_rounding=mode)
        for step in (1, 2):
            _set_grads(layers, step)
            before = [L.W_res.clone() for L in layers]
            cb = None if layers[1].W_c is None else layers[1].W_c.clone()
            st.step(LR, step)
            if mode == "compensated":
                w, c = comp_merge_reference(before[1], cb, _store_dw(ops, layers[0]._arena, 1, layers[1]))
                assert _same(layers[1].W_res, w) and _same(layers[1].W_c, c)
        runs[mode] = [L.W_res.clone() for L in layers]
        assert layers[0].W_c is None and (layers[1].W_c is not None) == (mode == "compensated")
        assert ops.comp_calls == ([128 * 192] * 2 if mode == "compensated" else [])
    assert torch.equal(runs["nearest"][0], runs["compensated"][0])
    assert not torch.equal(runs["nearest"][1], runs["compensated"][1])


# ------------------------------------------------------------------------------------------ the state
def test_state_dict_is_unchanged():
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    ops = CompCpuOps()
    model = _model(SHAPES, [torch.bfloat16] * 2)
    layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], 0, 1, R, float(R), ops=ops)
    keys = list(model.state_dict().keys())
    st = HDPissaStep(model, 1, 0, ops=ops, merge_rounding="compensated")
    _set_grads(layers, 1)
    st.step(LR, 1)
    assert layers[0].W_c.any()
    assert list(model.state_dict().keys()) == keys and not any("W_c" in k for k in keys)
    assert all(torch.equal(L.merge_weights(), L.W_res) for L in layers)


def test_rebuilt_stepper_keeps_the_compensation():
    from hdpissa_amd import HDPissaStep
    model, layers, st, ops = _build()
    _, ref_layers, ref, _ = _build()
    for step in (1, 2):
        _set_grads(ref_layers, step)
        ref.step(LR, step)
    _set_grads(layers, 1)
    st.step(LR, 1)
    held = [L.W_c for L in layers]
    st2 = HDPissaStep(model, 1, 0, ops=ops, exchange="allreduce", merge_rounding="compensated")
    assert all(L.W_c is h and h.any() for L, h in zip(layers, held))
    _set_grads(layers, 2)
    st2.step(LR, 2)
    for a, b in zip(layers, ref_layers):
        assert _same(a.W_res, b.W_res) and _same(a.W_c, b.W_c)
    layers[0].reset_compensation()
    assert not layers[0].W_c.any() and layers[1].W_c.any()


def test_written_w_res_restarts_that_layers_compensation():
    from hdpissa_amd.rounding import comp_merge_reference
    _, layers, st, ops = _build()
    _set_grads(layers, 1)
    st.step(LR, 1)
    assert all(L.W_c.any() for L in layers)
    with torch.no_grad():
        layers[0].W_res.copy_(layers[0].W_res.float() * 0.5)
    before = [(L.W_res.clone(), L.W_c.clone()) for L in layers]
    _set_grads(layers, 2)
    st.step(LR, 2)
    arena = layers[0]._arena
    w, c = comp_merge_reference(before[0][0], torch.zeros_like(before[0][1]), _store_dw(ops, arena, 0, layers[0]))
    assert _same(layers[0].W_res, w) and _same(layers[0].W_c, c)        # started from W_c = 0
    w, c = comp_merge_reference(*before[1], _store_dw(ops, arena, 1, layers[1]))
    assert _same(layers[1].W_res, w) and _same(layers[1].W_c, c)        # the other layer kept its term
    assert before[1][1].any()


# ------------------------------------------------------------------------------------------ resume
def test_resume_equals_straight_run(tmp_path):
    from hdpissa_amd import load_hdpissa_state, save_hdpissa_state
    _, la, sa, _ = _build()
    for step in (1, 2, 3):
        _set_grads(la, step)
        sa.step(LR, step)
    mb, lb, sb, _ = _build()
    for step in (1, 2):
        _set_grads(lb, step)
        sb.step(LR, step)
    path = str(tmp_path / "state.safetensors")
    save_hdpissa_state(mb, path, t=2)
    from hdpissa_amd import replace_with_custom_layer, HDPissaStep
    ops = CompCpuOps()
    mc = _model(SHAPES, [torch.bfloat16] * 2)  # a fresh model: W_c does not exist until the file brings it
    lc = replace_with_custom_layer(mc, [s[0] for s in SHAPES], 0, 1, R, float(R), ops=ops)
    assert all(L.W_c is None for L in lc)
    assert load_hdpissa_state(mc, path) == 2
    for b, c in zip(lb, lc):
        assert _same(b.W_c, c.W_c) and c.W_c.any() and c._comp_version == c.W_res._version
    sc = HDPissaStep(mc, 1, 0, ops=ops, merge_rounding="compensated")
    _set_grads(lc, 3)
    sc.step(LR, 3)
    for a, c in zip(la, lc):
        assert _same(a.W_res, c.W_res) and _same(a.W_c, c.W_c)


def test_nearest_file_loads_with_zero_compensation_and_keeps_its_names(tmp_path):
    from safetensors import safe_open
    from hdpissa_amd import load_hdpissa_state, save_hdpissa_state
    mn, ln, sn, _ = _build(merge_rounding="nearest")
    _set_grads(ln, 1)
    sn.step(LR, 1)
    path = str(tmp_path / "nearest.safetensors")
    save_hdpissa_state(mn, path, t=1)
    with safe_open(path, framework="pt") as f:
        assert sorted(f.keys()) == sorted(["arena0.fac_all", "arena0.m", "arena0.v", "arena0.grad", "q_proj.W_res",
                                           "o_proj.W_res"])
        assert f.metadata()["format"] == "hdpissa-resume-1"
    mc, lc, sc, _ = _build()
    _set_grads(lc, 1)
    sc.step(LR, 1)
    assert all(L.W_c.any() for L in lc)
    assert load_hdpissa_state(mc, path) == 1
    for n, c in zip(ln, lc):
        assert _same(n.W_res, c.W_res) and not c.W_c.any() and c._comp_version == c.W_res._version
    path2 = str(tmp_path / "comp.safetensors")
    save_hdpissa_state(mc, path2, t=1)
    with safe_open(path2, framework="pt") as f:
        assert {"q_proj.W_c", "o_proj.W_c"} <= set(f.keys()) and f.metadata()["format"] == "hdpissa-resume-1"


# ------------------------------------------------------------------------------------------ the reason for it
def test_compensation_keeps_the_update():
    """One bf16 layer 128 x 192, r 16, lr 5e-5, the same gradients before each of 128 steps (the inputs of
    tests/test_gpu_merge_comp.py's drift test), through the CPU op set.  err(x) = ||x - (W0 + sum dW)|| / ||sum dW||,
    sum dW from a float32-W copy of the layer on the same factors.  Required: err(nearest) >= 0.8,
    err(W_res, compensated) <= 0.5 err(stochastic), err(float32(W_res) + float32(W_c)) <= 0.5 err(W_res,
    compensated).  This CPU run gave: nearest 0.8996, stochastic 0.2289, compensated W_res 0.0269 (0.12 of
    stochastic), W_res + W_c 0.0029 (0.11 of W_res alone)."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    lr, steps, shapes = 5e-5, 128, [("q_proj", 128, 192)]

    def build(dt, **kw):
        ops = CompCpuOps()
        model = _model(shapes, [dt])
        (L,) = replace_with_custom_layer(model, ["q_proj"], 0, 1, 16, 16.0, ops=ops)
        return L, (lambda: HDPissaStep(model, 1, 0, ops=ops, **kw))

    def run(L, st):
        g = torch.Generator().manual_seed(77)
        gA, gB = (torch.randn(s, generator=g) * 1e-14 for s in (L.A.shape, L.B.shape))
        for t in range(1, steps + 1):
            L.A.grad, L.B.grad = gA.clone(), gB.clone()
            st.step(lr, t)
        return L.W_res.float().numpy().astype(np.float64)

    Lf, mk = build(torch.float32)
    W0 = Lf.W_res.float().numpy().astype(np.float64)
    Wf = run(Lf, mk())
    total = np.linalg.norm(Wf - W0)
    err = {}
    for mode, kw in (("nearest", {}), ("stochastic", dict(merge_rounding="stochastic", sr_seed=20240607)),
                     ("compensated", dict(merge_rounding="compensated"))):
        L, mk = build(torch.bfloat16, **kw)
        with torch.no_grad():
            L._arena.fac_all.copy_(Lf._arena.fac_all)  # the very same factors
        assert np.array_equal(L.W_res.float().numpy().astype(np.float64), W0)
        err[mode] = float(np.linalg.norm(run(L, mk()) - Wf) / total)
        if mode == "compensated":
            both = L.W_res.float().numpy().astype(np.float64) + L.W_c.float().numpy().astype(np.float64)
            err["compensated W+C"] = float(np.linalg.norm(both - Wf) / total)
    print("128 steps at lr 5e-5: " + ", ".join(f"{k} {v:.4f}" for k, v in err.items()))
    assert err["nearest"] >= 0.8, err
    assert err["compensated"] <= 0.5 * err["stochastic"], err
    assert err["compensated W+C"] <= 0.5 * err["compensated"], err

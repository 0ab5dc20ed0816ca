"""compute_dtype=torch.bfloat16 on the device: float32 master weights, a bf16 copy for the base GEMMs.

The layer under bf16 autocast (y, dX and the probe gradients against float64 formulas on the bf16-rounded x, W
and gy: 2e-2 relative for the bf16 GEMM outputs, 1e-5 for the gradients -- test_gpu_layer.py's bars), and the
step's contract: when step() returns, W_lp is bf16(W_res) (the host replica rounding.rne_bf16_bits) element for
element and W_res is bitwise what a twin model without the copy gets from the same gradients -- under every
exchange, with and without max_grad_norm, in a mixed float32 / bf16 model, in residual mode, and at Wn = 2 as
two processes on the one GPU.  Last, a tiny Qwen2 through HDPissaTrainer(compute_dtype=) under autocast.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [("q_proj", 75, 130), ("up_proj", 128, 192)]  # ragged (in % 8 != 0, odd out) and tile-sized


def _replica(W):
    from hdpissa_amd.rounding import rne_bf16_bits
    bits = rne_bf16_bits(W.detach().contiguous().cpu().numpy().view(np.uint32)).astype(np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(W.shape)


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int16)


def _linear(inn, out, bias, seed, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    lin = nn.Linear(inn, out, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
        if bias:
            lin.bias.copy_(torch.randn(out, generator=g) * 0.1)
    return lin.to(DEV).to(dt).requires_grad_(False)


def _model(wn, rank, compute_dtype, comm=None, bf16_modules=(), residual=False):
    from hdpissa_amd import replace_with_custom_layer
    m = nn.Module()
    shapes = SHAPES + [("k_proj", 64, 130), ("o_proj", 96, 72)]
    for j, (name, out, inn) in enumerate(shapes):
        setattr(m, name, _linear(inn, out, False, 10 + j, BF if name in bf16_modules else torch.float32))
    layers = replace_with_custom_layer(m, [s[0] for s in shapes], rank, wn, 16, 16.0, comm=comm, residual=residual,
                                       compute_dtype=compute_dtype)
    return m, layers


def _feed(layers, step):
    for j, L in enumerate(layers):
        g = torch.Generator().manual_seed(100 * step + j)
        L.A.grad = (torch.randn(L.A.shape, generator=g) * 1e-14).to(DEV)
        L.B.grad = (torch.randn(L.B.shape, generator=g) * 1e-14).to(DEV)


def _check_copies(layers, tag):
    torch.cuda.synchronize()
    for L in layers:
        if L.W_res.dtype != torch.float32:
            assert L.W_lp is None, (tag, L.name)
            continue
        assert L.W_lp is not None and L.W_lp.dtype == BF
        assert torch.equal(_bits(L.W_lp), _replica(L.W_res)), (tag, L.name)


def _two_steps(wn, rank, exchange, clip, comms=(None, None), **model_kw):
    """Two steps of a shadowed model and its twin without the copy, fed the same gradients."""
    from hdpissa_amd import HDPissaStep
    m, layers = _model(wn, rank, BF, comm=comms[0], **model_kw)
    m0, layers0 = _model(wn, rank, None, comm=comms[1], **model_kw)
    _check_copies(layers, "init")
    W0 = [L.W_res.clone() for L in layers]
    kw = dict(exchange=exchange, bucket_bytes=60_000, max_grad_norm=clip)
    st = HDPissaStep(m, wn, rank, comm=comms[0], **kw)
    st0 = HDPissaStep(m0, wn, rank, comm=comms[1], **kw)
    for step in (1, 2):
        _feed(layers, step)
        _feed(layers0, step)
        st.step(1e-3, step)
        st0.step(1e-3, step)
        _check_copies(layers, (exchange, step))
        for L, L0 in zip(layers, layers0):
            assert torch.equal(L.W_res, L0.W_res), (exchange, step, L.name)
    assert all(not torch.equal(L.W_res, w) for L, w in zip(layers, W0))  # (the steps moved every W)
    return layers


@pytest.mark.parametrize("T", [17, 33])
@pytest.mark.parametrize("name,out,inn", SHAPES)
def test_layer_under_autocast(name, out, inn, T):
    """Forward and backward of a float32 layer on its bf16 copy, then a step driven by those gradients."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    m = nn.Module()
    setattr(m, name, _linear(inn, out, True, 1))
    (L,) = replace_with_custom_layer(m, [name], 0, 1, 16, 16.0, compute_dtype=BF)
    _check_copies([L], "init")
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, inn, generator=g).to(DEV).requires_grad_(True)
    gy = torch.randn(T, out, generator=g).to(DEV)
    with torch.autocast("cuda", dtype=BF):
        y = L(x)
    assert y.dtype == BF
    y.backward(gy.to(BF))
    torch.cuda.synchronize()
    assert x.grad.dtype == torch.float32
    xb, Wb, gb = x.detach().to(BF).double().cpu(), L.W_lp.double().cpu(), gy.to(BF).double().cpu()
    y_ref = xb @ Wb.T + L.bias.detach().to(BF).double().cpu()
    A, B, s = L.A.detach().double().cpu(), L.B.detach().double().cpu(), L.probe_scale
    errs = dict(y=rel_err(y.detach().float().cpu().numpy(), y_ref.numpy()),
                dX=rel_err(x.grad.cpu().numpy(), (gb @ Wb).numpy()),
                gA=rel_err(L.A.grad.cpu().numpy(), (s * (gb @ B).T @ xb).numpy()),
                gB=rel_err(L.B.grad.cpu().numpy(), (s * gb.T @ (xb @ A.T)).numpy()))
    print(name, T, {k: f"{v:.3e}" for k, v in errs.items()})
    assert errs["y"] < 2e-2 and errs["dX"] < 2e-2
    assert errs["gA"] < 1e-5 and errs["gB"] < 1e-5
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        assert torch.equal(L(x.detach()), y.detach())  # the no-grad forward runs the same GEMM
    W0 = L.W_res.clone()
    HDPissaStep(m, 1, 0).step(1e-2, 1)
    _check_copies([L], "step")
    assert not torch.equal(L.W_res, W0)


def test_shared_activation_reaches_the_probe_once():
    """q / k / v handed one float32 x save one bf16 tensor, so the grouped probe sees one X."""
    from hdpissa_amd import replace_with_custom_layer
    m = nn.Module()
    m.q_proj, m.k_proj, m.v_proj = _linear(130, 96, False, 1), _linear(130, 32, False, 2), _linear(130, 32, False, 3)
    layers = replace_with_custom_layer(m, ["q_proj", "k_proj", "v_proj"], 0, 1, 16, 16.0, compute_dtype=BF)
    x = torch.randn(2, 17, 130, generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.autocast("cuda", dtype=BF):
        ys = [L(x) for L in layers]
    saved = [y.grad_fn.saved_tensors[0] for y in ys]
    assert all(s.dtype == BF and s.data_ptr() == saved[0].data_ptr() for s in saved)
    sum(y.float().sum() for y in ys).backward()
    torch.cuda.synchronize()
    assert layers[0]._arena.cast_cache is None
    xb = x.to(BF).double().cpu().reshape(-1, 130)
    for L in layers:
        gb = torch.ones(xb.shape[0], L.out_features, dtype=torch.float64)
        A, B, s = L.A.detach().double().cpu(), L.B.detach().double().cpu(), L.probe_scale
        assert rel_err(L.A.grad.cpu().numpy(), (s * (gb @ B).T @ xb).numpy()) < 1e-5
        assert rel_err(L.B.grad.cpu().numpy(), (s * gb.T @ (xb @ A.T)).numpy()) < 1e-5


@pytest.mark.parametrize("clip", [None, float("inf")])
@pytest.mark.parametrize("exchange", ["gather", "allreduce", "shard"])
def test_step_keeps_the_copy_current(exchange, clip):
    _two_steps(1, 0, exchange, clip)


@pytest.mark.parametrize("exchange", ["gather", "allreduce"])
def test_mixed_model(exchange):
    """bf16 modules between the float32 ones keep no copy and merge as they always did."""
    layers = _two_steps(1, 0, exchange, None, bf16_modules=("up_proj", "o_proj"))
    assert [L.W_lp is None for L in layers] == [False, True, False, True]


def test_skipped_step():
    """A non-finite gradient norm: W_res stays, and the copy is still cast from it."""
    from hdpissa_amd import HDPissaStep
    m, layers = _model(1, 0, BF)
    st = HDPissaStep(m, 1, 0, max_grad_norm=1.0)
    _feed(layers, 1)
    layers[1].B.grad[0, 0] = float("nan")
    for L in layers:
        L.W_res.data.mul_(1.25)  # (behind the version counter's back)
    W0 = [L.W_res.clone() for L in layers]
    st.step(1e-3, 1)
    _check_copies(layers, "skipped")
    assert st.clip_info()["skipped"]
    assert all(torch.equal(L.W_res, w) for L, w in zip(layers, W0))


def test_residual_mode():
    """make_residual rewrites W_res through K4: the copy follows, and the forward adds the frozen components
    computed from the original x."""
    layers = _two_steps(1, 0, "gather", None, residual=True)
    m = nn.Module()
    m.q_proj = _linear(130, 75, False, 10)
    W0 = m.q_proj.weight.clone()
    from hdpissa_amd import replace_with_custom_layer
    (L,) = replace_with_custom_layer(m, ["q_proj"], 0, 1, 16, 16.0, residual=True, compute_dtype=BF)
    _check_copies([L], "residual init")
    assert not torch.equal(L.W_res, W0)
    x = torch.randn(17, 130, generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.autocast("cuda", dtype=BF):
        y = L(x)
    assert rel_err(y.detach().float().cpu().numpy(), (x @ W0.T).cpu().numpy()) < 2e-2
    assert layers[0].residual


def _worker(rank, wn, port, errfile):
    import sys
    import torch.distributed as dist
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        from test_gpu_ranks_one_gpu import HostComm
        for exchange in ("gather", "allreduce", "shard"):
            layers = _two_steps(wn, rank, exchange, None, comms=(HostComm(rank, wn), HostComm(rank, wn)))
            for L in layers:
                w, lp = L.W_res.cpu(), _bits(L.W_lp).reshape(-1).view(torch.uint8).clone()  # (gloo: no 16-bit gather)
                ws, lps = [torch.zeros_like(w) for _ in range(wn)], [torch.zeros_like(lp) for _ in range(wn)]
                dist.all_gather(ws, w)
                dist.all_gather(lps, lp)
                same_w = all(torch.equal(ws[0], x) for x in ws)
                assert same_w or exchange == "allreduce", (exchange, L.name)  # (float32 all-reduce: not bitwise)
                if same_w:
                    assert all(torch.equal(lps[0], x) for x in lps), (exchange, L.name)
    except Exception as e:  # surface the assertion text to the parent
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu(tmp_path):
    """Wn = 2 as two processes sharing the GPU (gloo on host copies), the three exchanges in turn."""
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    errfile = str(tmp_path / "err.txt")
    try:
        mp.spawn(_worker, args=(2, port, errfile), nprocs=2, join=True)
    except Exception:
        pytest.fail("worker failed:\n" + (open(errfile).read() if os.path.exists(errfile) else ""))


# |first loss (bf16 compute) - first loss (float32)| of this model and these batches, measured on the CPU with
# the test op set under torch.autocast("cpu"): 1.19e-6 (5.5258760 against 5.5258772: the tiny model's logits
# are near zero, so the loss sits at ln 256 and hardly feels the bf16 rounding).  The margin is twice that.
LOSS_MARGIN = 2.4e-6


def test_tiny_qwen2_trainer_under_autocast():
    """2 steps x 2 micro-batches of the trajectory fixture's tiny Qwen2: HDPissaTrainer(compute_dtype=) runs
    the model under autocast on the layers' bf16 copies; the float32 run of the same model is the yardstick."""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    from helpers import QWEN_TARGETS, QWEN_TINY
    from hdpissa_amd import HDPissaTrainer, replace_with_custom_layer
    z = np.load(os.path.join(HERE, "golden", "trajectory_qwen2_w1.npz"))

    def run(cd):
        model = Qwen2ForCausalLM(Qwen2Config(**QWEN_TINY, attn_implementation="eager")).float()
        model.load_state_dict({k[len("state."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("state.")})
        model = model.to(DEV)
        for p in model.parameters():
            p.requires_grad = False
        layers = replace_with_custom_layer(model, QWEN_TARGETS, 0, 1, int(z["r"]), float(z["alpha"]), compute_dtype=cd)
        tr = HDPissaTrainer(model, 1, 0, float(z["lr"]), 2, 2, compute_dtype=cd)
        for i in range(4):
            tr.micro_step({k: torch.from_numpy(z[f"r0.mb{i}.{k}"]) for k in ("input_ids", "labels", "attention_mask")})
        torch.cuda.synchronize()
        return tr.loss_list, layers

    ref, _ = run(None)
    got, layers = run(BF)
    print("losses float32", ref, "bf16 compute", got, "first-loss difference", abs(got[0] - ref[0]))
    assert len(got) == 2 and all(np.isfinite(got))
    _check_copies(layers, "trainer")
    assert all(L.W_lp is not None for L in layers)
    assert abs(got[0] - ref[0]) <= LOSS_MARGIN

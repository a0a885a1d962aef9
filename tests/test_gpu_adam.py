"""-m gpu: the Adam branch on the device step — paa_adam_step against torch.optim.Adam, PgdStepper(optimizer=...) eager vs
captured, two gloo ranks vs one, one rank over RCCL, and the drop-in runner with two ranks (train.py:165-175, build.py:352-359)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = ["ab cd", "hello", "a b c", "xyz w"]


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("L,offset", [(4097, 0), (8000, 0), (8000, 1), (160000, 0)])
@pytest.mark.parametrize("grad_sign", [1.0, -1.0])
def test_adam_step_matches_torch_adam(L, offset, grad_sign):
    """50 steps of paa_adam_step next to torch.optim.Adam fed the same p.grad, lr halved after step 20 as StepLR would;
    gradients spread over 1e-8 .. 1e-1.  offset=1 puts every vector off 16-byte alignment (the element-wise path)."""
    from paa_amd import _lib
    from paa_amd.training_utils.pgd import adam_scalars
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(L + offset + int(grad_sign > 0))
    p0 = torch.randn(L, generator=gen) * 1e-2
    grads = [torch.pow(10.0, torch.rand(L, generator=gen) * 7 - 8) * torch.randn(L, generator=gen).sign() for _ in range(50)]
    p_t = torch.nn.Parameter(p0.clone().to(dev))
    opt = torch.optim.Adam([p_t], lr=1e-3)
    buf = torch.zeros(5, L + offset, device=dev)
    p, g, m, v, gout = (buf[i, offset:] for i in range(5))
    p.copy_(p0)
    scal = torch.zeros(2, device=dev)
    lib = _lib.lib()
    for t, gr in enumerate(grads, start=1):
        if t == 21:
            opt.param_groups[0]["lr"] *= 0.5
        gr = gr.to(dev)
        p_t.grad = grad_sign * gr
        opt.step()
        g.copy_(gr)
        grp = opt.param_groups[0]
        b1, b2 = grp["betas"]
        scal.copy_(torch.tensor(adam_scalars(grp["lr"], b1, b2, float(t)), dtype=torch.float32))
        _lib.check(lib.paa_adam_step(_lib.ptr(p), _lib.ptr(g), grad_sign, _lib.ptr(m), _lib.ptr(v), _lib.ptr(scal),
                                     float(1 - b1), float(b2), float(1 - b2), float(grp["eps"]), _lib.ptr(gout), L,
                                     _lib.stream_ptr()))
    torch.cuda.synchronize()
    st = opt.state[p_t]
    assert float(st["step"]) == 50
    pairs = {"p": (p, p_t.detach()), "exp_avg": (m, st["exp_avg"]), "exp_avg_sq": (v, st["exp_avg_sq"]), "grad": (gout, p_t.grad)}
    for k, (a, b) in pairs.items():
        print(f"L={L} offset={offset} sign={grad_sign:+.0f} {k}: bit-equal {torch.equal(a, b)}, "
              f"max abs diff {float((a - b).abs().max()):.3e}")
    for k, (a, b) in pairs.items():
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-3 * 1e-6 if k == "p" else 0.0)
    # the contractions were matched to torch's gfx950 foreach kernels: the result is the same bits
    for k, (a, b) in pairs.items():
        assert torch.equal(a, b), k


def _adam_setup(norm, B, L, first=0, lr=2e-4):
    from oracle.gen_cases import cli_to_args
    from paa_amd import arch as A, synth
    from paa_amd.model import PaaModel
    from paa_amd.training_utils import build
    args = cli_to_args(norm, ["--snr_db", "40"] if norm == "snr" else [])
    args.device, args.optimizer_type, args.lr, args.step_size, args.gamma = "cuda", "adam", lr, 1, 0.5
    clean = torch.from_numpy(synth.clean_audio(B, L, first_clip=first)).cuda()
    p = torch.nn.Parameter(torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L))
    opt, sched = build.create_optimizer(args, p)
    m = PaaModel(A.tiny(), A.rule_weights(A.tiny()), B, L, "fp32")
    return args, clean, p, opt, sched, m


def test_adam_stepper_capture_equals_eager():
    from oracle import pgd as opgd
    from paa_amd.training_utils.pgd import PgdStepper
    B, L, steps = 2, 8000, 3
    runs = {}
    for mode in ("eager", "graph"):
        args, clean, p, opt, sched, m = _adam_setup("snr", B, L)
        labels = opgd.make_labels(TEXTS[:B], args, B)
        st = PgdStepper(m, args, L, optimizer=opt)
        if mode == "eager":
            for i in range(steps):
                st.step(p.data, clean, labels)
                sched.step()
        else:
            p0 = p.detach().clone()
            g, _ = st.capture(p.data, clean, labels)
            assert not isinstance(g, torch.cuda.CUDAGraph) and hasattr(g, "replay")
            torch.cuda.synchronize()
            assert torch.equal(p.detach(), p0) and float(opt.state[p]["step"]) == 0      # capture() takes no step
            for i in range(steps):
                g.replay()
                sched.step()
        torch.cuda.synchronize()
        s = opt.state[p]
        assert float(s["step"]) == steps and opt.param_groups[0]["lr"] == pytest.approx(2e-4 * 0.5 ** steps)
        runs[mode] = (p.detach().clone(), s["exp_avg"].clone(), s["exp_avg_sq"].clone(), p.grad.clone())
        if mode == "graph":
            opt.param_groups[0]["betas"] = (0.8, 0.999)
            with pytest.raises(ValueError):
                g.replay()
    for a, b in zip(runs["eager"], runs["graph"]):
        assert torch.equal(a, b)
    assert float(runs["eager"][1].abs().max()) > 0


def _dp_worker(rank, world, port, norm, q, sizes, graph):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from oracle import pgd as opgd
    from paa_amd.training_utils.pgd import PgdStepper
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    B, L = sizes[rank], 8000
    first = sum(sizes[:rank])
    args, clean, p, opt, sched, m = _adam_setup(norm, B, L, first)
    labels = opgd.make_labels(TEXTS[first:first + B], args, B)
    st = PgdStepper(m, args, L, optimizer=opt)
    assert st.world == world and st.collective
    if graph:
        g, _ = st.capture(p.data, clean, labels)
        step = g.replay
    else:
        def step():
            st.step(p.data, clean, labels)
    for _ in range(3):
        step()
        sched.step()
    torch.cuda.synchronize()
    out = [torch.zeros_like(p.data) for _ in range(world)]
    dist.all_gather(out, p.data)
    if rank == 0:
        q.put((p.detach().cpu().numpy(), float(st.stats[0]), all(torch.equal(o, out[0]) for o in out),
               float(opt.state[p]["step"])))
    dist.destroy_process_group()


@pytest.mark.parametrize("norm,sizes,graph", [("snr", (2, 2), False), ("max_phon", (2, 2), False), ("snr", (3, 1), False),
                                              ("snr", (2, 2), True), ("snr", (3, 1), True), ("max_phon", (2, 2), True)])
def test_adam_two_ranks_equal_one(norm, sizes, graph):
    """Two gloo ranks on the one GPU, three Adam steps with StepLR between them: replicas bit-identical, and equal to one
    rank on the global batch except where a gradient entry is numerically ~0 (its sign, and so its Adam step, is decided by
    the summation order of the shards)."""
    from oracle import pgd as opgd
    from paa_amd.training_utils.pgd import PgdStepper
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, norm, q, sizes, graph)) for r in range(2)]
    for pr in procs:
        pr.start()
    p_dp, loss_dp, identical, nsteps = q.get(timeout=300)
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    assert identical and nsteps == 3
    B, L = 4, 8000
    args, clean, p, opt, sched, m = _adam_setup(norm, B, L)
    st = PgdStepper(m, args, L, optimizer=opt)
    labels = opgd.make_labels(TEXTS, args, B)
    for _ in range(3):
        st.step(p.data, clean, labels)
        sched.step()
    torch.cuda.synchronize()
    assert loss_dp == pytest.approx(float(st.stats[0]), rel=1e-5)
    ref = p.detach().cpu().numpy()
    diff = np.abs(p_dp - ref)
    scale = np.abs(ref).max()
    print(f"adam {norm} {sizes} graph={graph}: DP vs single max diff {diff.max() / scale:.2e}; "
          f"fraction differing {(diff > 1e-6 * scale).mean():.2e}")
    assert (diff > 1e-5 * scale).mean() < 1e-2


def test_adam_one_rank_rccl():
    """force_collective=True on one rank over "nccl" (RCCL), eager and captured (two graphs around the collective), in a fresh
    child interpreter: with one rank the sum is the identity, so the Adam trajectory must equal the collective-free stepper's
    (bit for bit for max_phon; snr takes sum clean^2 from the all-reduced vector, one f32 rounding earlier)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = json.loads([line for line in r.stdout.splitlines() if line.startswith("ADAM_RCCL ")][-1][len("ADAM_RCCL "):])
    print(d)
    assert d["backend"] == "nccl" and d["world"] == 1
    mp_, snr = d["max_phon"], d["snr"]
    assert mp_["graph_type"] == "_SplitGraph" and snr["graph_type"] == "_SplitGraph"
    assert mp_["eager_equal"] and mp_["graph_equal"], mp_
    assert snr["graph_equals_eager_collective"], snr
    assert snr["eager_maxdiff"] < 1e-5 and snr["graph_maxdiff"] < 1e-5, snr
    for c in (mp_, snr):
        assert c["steps"] == 3.0


def _rccl_child():
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    from oracle import pgd as opgd
    from paa_amd.training_utils.pgd import PgdStepper
    B, L, steps = 3, 8000, 3
    out = {"backend": dist.get_backend(), "world": dist.get_world_size()}
    for norm in ("max_phon", "snr"):
        res = {}
        for mode in ("plain", "eager", "graph"):
            args, clean, p, opt, sched, m = _adam_setup(norm, B, L)
            labels = opgd.make_labels(TEXTS[:B], args, B)
            st = PgdStepper(m, args, L, force_collective=mode != "plain", optimizer=opt)
            step = lambda: st.step(p.data, clean, labels)      # noqa: E731
            if mode == "graph":
                g, _ = st.capture(p.data, clean, labels)
                res["graph_type"] = type(g).__name__
                step = g.replay
            for _ in range(steps):
                step()
                sched.step()
            torch.cuda.synchronize()
            res[mode] = p.detach().clone()
            res["steps"] = float(opt.state[p]["step"])
        scale = float(res["plain"].abs().max())
        out[norm] = {"eager_equal": bool(torch.equal(res["eager"], res["plain"])),
                     "graph_equal": bool(torch.equal(res["graph"], res["plain"])),
                     "graph_equals_eager_collective": bool(torch.equal(res["graph"], res["eager"])),
                     "eager_maxdiff": float((res["eager"] - res["plain"]).abs().max()) / scale,
                     "graph_maxdiff": float((res["graph"] - res["plain"]).abs().max()) / scale,
                     "graph_type": res["graph_type"], "steps": res["steps"]}
    dist.destroy_process_group()
    print("ADAM_RCCL " + json.dumps(out), flush=True)


_RUNNER_FLAGS = ["--arch", "tiny", "--audio_seconds", "0.5", "--steps_per_epoch", "2", "--num_epochs", "2", "--dtype", "fp32",
                 "--silent", "--optimizer_type", "adam", "--norm_type", "snr", "--snr_db", "40", "--step_size", "1",
                 "--gamma", "0.5"]


def _runner_worker(rank, world, port, logs, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      PAA_DIST_BACKEND="gloo")
    from paa_amd import run_attack
    from paa_amd.training_utils import parser
    args = parser.create_arg_parser().parse_args(_RUNNER_FLAGS + ["--batch_size", "2", "--logs_dir", logs])
    rc = run_attack.main(args)
    q.put((rank, rc, args.save_dir))
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def test_runner_two_ranks_adam_matches_one_rank(tmp_path):
    """The runner with WORLD_SIZE=2 (gloo, both ranks on the one GPU) and the Adam branch with StepLR: it finishes, and rank
    0's results.json / perturbation.pt equal those of one rank on the same global batches up to the shards' summation order."""
    from paa_amd import run_attack
    from paa_amd.training_utils import parser
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_runner_worker, args=(r, 2, port, str(tmp_path / "dp2"), q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=600) for _ in range(2))
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    assert [r[1] for r in res] == [0, 0]
    d2 = json.load(open(os.path.join(res[0][2], "results.json")))
    p2 = torch.load(os.path.join(res[0][2], "perturbation.pt"), weights_only=True)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    args = parser.create_arg_parser().parse_args(_RUNNER_FLAGS + ["--batch_size", "4", "--logs_dir", str(tmp_path / "dp1")])
    assert run_attack.main(args) == 0
    d1 = json.load(open(os.path.join(args.save_dir, "results.json")))
    p1 = torch.load(os.path.join(args.save_dir, "perturbation.pt"), weights_only=True)
    print("DP2 results:", json.dumps(d2))
    print("one-rank results:", json.dumps(d1))
    assert d2["finished_training"] == 1.0 and d2["best_epoch"] == d1["best_epoch"]
    for key in ("final_test_perturbed", "final_test_clean", "best_train_score"):
        for m_ in ("ctc", "wer"):
            assert d2[key][m_] == pytest.approx(d1[key][m_], rel=2e-3, abs=1e-6), (key, m_, d2[key], d1[key])
    diff = (p2 - p1).abs().numpy()
    scale = float(p1.abs().max())
    print(f"runner Adam DP2 vs one rank: p max diff {diff.max() / scale:.2e}, fraction differing {(diff > 1e-5 * scale).mean():.2e}")
    assert (diff > 1e-5 * scale).mean() < 2e-2


if __name__ == "__main__":
    _rccl_child()

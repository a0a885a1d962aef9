"""Child process of tests/test_gpu_chan.py (started fresh): ONE rank of a two-rank gloo group, both ranks on cuda:0.  The rank holds
one clip and DRAWS its channel under the global clip id rank * max_batch + b; it takes two eager steps, then
two replayed steps of the two-graph form from the same start and the same counters, writes its perturbations to
<out_dir>/rank<r>.npz and prints one JSON line.

    python chan_dist_child.py RANK WORLD PORT OUT_DIR
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTS = ["ab cd", "hello"]
L, STEPS = 8000, 2
DRIFT_PPM, NOISE = 20000.0, (20.0, 30.0)


def case_args():
    from oracle.gen_cases import cli_to_args
    args = cli_to_args("linf", ["--linf_size", "0.01"])
    args.device = "cuda"
    args.sr, args.seed = 16000, 5
    args.drift_ppm, args.noise_snr_db = DRIFT_PPM, list(NOISE)
    return args


def main():
    rank, world, port, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    import numpy as np
    import torch
    import torch.distributed as dist
    from oracle import pgd as opgd
    from paa_amd import arch as A, synth
    from paa_amd.model import PaaModel
    from paa_amd.training_utils.pgd import PgdStepper
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    a = A.tiny()
    args = case_args()
    clean = torch.from_numpy(synth.clean_audio(1, L, first_clip=rank)).cuda()
    p0 = torch.from_numpy(synth.perturbation(L) * np.float32(1e-2)).cuda().view(1, L)
    labels = opgd.make_labels(TEXTS[rank:rank + 1], args, 1)
    m = PaaModel(a, A.rule_weights(a), 1, L, "fp32")
    st = PgdStepper(m, args, L)
    assert st.world == world and st.collective and st.chan_on and not st.place_on and st.clip_base == rank
    assert st.chan.clip_base == rank
    p_e = p0.clone()
    rq = []
    for _ in range(STEPS):
        r = st.step(p_e, clean, labels)
        rq.append(int(st.chan.rq[0].item()))
    torch.cuda.synchronize()
    loss_e = float(r["loss"])
    p_g = p0.clone()
    st.set_chan_step(0)                                  # the replays hear what the eager steps heard
    g, _ = st.capture(p_g, clean, labels)
    p_g.copy_(p0)
    for _ in range(STEPS):
        g.replay()
    torch.cuda.synchronize()
    gathered = [torch.zeros_like(p_e) for _ in range(world)]
    dist.all_gather(gathered, p_e)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), p_eager=p_e.cpu().numpy(), p_graph=p_g.cpu().numpy())
    out = {"rank": rank, "loss": loss_e, "replicas_identical": all(torch.equal(o, gathered[0]) for o in gathered),
           "graph_equals_eager": bool(torch.equal(p_g, p_e)), "split_graph": type(g).__name__, "rq": rq,
           "counters": [int(st.chan.counter.item()), int(st.chan.noise_counter.item())]}
    dist.barrier()
    dist.destroy_process_group()
    print("CHAN_CHILD " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Child process of tests/test_gpu_rir.py (started fresh): ONE rank of a two-rank gloo group, both ranks on cuda:0.  The rank holds
one clip, an explicit placement and an explicit room of its own; it takes two eager steps, then two replayed
steps of the two-graph form from the same start, writes its perturbations to <out_dir>/rank<r>.npz and prints one JSON line.

    python rir_dist_child.py RANK WORLD PORT OUT_DIR
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTS = ["ab cd", "hello"]
SHIFTS = (5555, 143)
ROOMS = (3, 1)
L, STEPS = 8000, 2


def case_args():
    from oracle.gen_cases import cli_to_args
    args = cli_to_args("snr", ["--snr_db", "40"])
    args.device = "cuda"
    args.perturbation_seconds = L / 16000          # placement on, Lp = L (snr needs it)
    args.sr, args.seed = 16000, 5
    args.rir_bank, args.rir_count, args.rir_taps = "synthetic", 4, 300
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
    assert st.world == world and st.collective and st.place_on and st.rir_on and st.clip_base == rank
    assert st.reverb.clip_base == rank
    st.set_placement([SHIFTS[rank]])
    st.set_rooms([ROOMS[rank]])
    p_e = p0.clone()
    for _ in range(STEPS):
        r = st.step(p_e, clean, labels)
    torch.cuda.synchronize()
    loss_e = float(r["loss"])
    p_g = p0.clone()
    g, _ = st.capture(p_g, clean, labels)
    p_g.copy_(p0)
    for _ in range(STEPS):
        g.replay()
    torch.cuda.synchronize()
    gathered = [torch.zeros_like(p_e) for _ in range(world)]
    dist.all_gather(gathered, p_e)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), p_eager=p_e.cpu().numpy(), p_graph=p_g.cpu().numpy())
    out = {"rank": rank, "loss": loss_e, "replicas_identical": all(torch.equal(o, gathered[0]) for o in gathered),
           "graph_equals_eager": bool(torch.equal(p_g, p_e)), "split_graph": type(g).__name__}
    dist.barrier()
    dist.destroy_process_group()
    print("RIR_CHILD " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Child process of tests/test_gpu_varlen_model.py (started fresh): ONE rank of a two-rank gloo group, both ranks on cuda:0.  The
rank holds one clip with a true length of its own, takes two universal steps under lengths, writes its perturbation to
<out_dir>/rank<r>.npz and prints one JSON line.

    python varlen_dist_child.py RANK WORLD PORT OUT_DIR
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXTS = ["ab cd", "hello"]
LENGTHS = (5321, 3000)
L, STEPS = 8000, 2


def case_args():
    from oracle.gen_cases import cli_to_args
    args = cli_to_args("snr", ["--snr_db", "40"])
    args.device = "cuda"
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
    a = A.tiny("group", False, hidden_size=128, num_attention_heads=2, intermediate_size=256)      # head dim 64: fused attention
    args = case_args()
    clean = torch.from_numpy(synth.clean_audio(1, L, first_clip=rank)).cuda()
    p = torch.from_numpy(synth.perturbation(L).reshape(1, L) * np.float32(1e-2)).cuda()
    labels = opgd.make_labels(TEXTS[rank:rank + 1], args, 1)
    m = PaaModel(a, A.rule_weights(a), 1, L, "fp32")
    st = PgdStepper(m, args, L)
    assert st.world == world and st.collective
    for _ in range(STEPS):
        r = st.step(p, clean, labels, lengths=[LENGTHS[rank]])
    torch.cuda.synchronize()
    gathered = [torch.zeros_like(p) for _ in range(world)]
    dist.all_gather(gathered, p)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), p=p.cpu().numpy())
    out = {"rank": rank, "loss": float(r["loss"]), "replicas_identical": all(torch.equal(o, gathered[0]) for o in gathered)}
    dist.barrier()
    dist.destroy_process_group()
    print("VARLEN_CHILD " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""Stop and go on with more than one rank, on the CPU: 2 gloo ranks train 2 steps, every rank saves its training state to its own file,
fresh models and fresh trainers load them and train 2 more steps.  The result must be the uninterrupted 2-rank run's, bit for bit, and
the same on both ranks — in the staged form on the fp32 wire and on the bf16 wire (whose buffer is scratch: it is not saved)."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

CONFIGS = [("f32", True), ("bf16", True), ("f32", False)]


class Toy(nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.a = nn.Linear(7, 15)
        self.dead = nn.Linear(15, 15)
        self.b = nn.Linear(15, 3)
        self.s = nn.Parameter(torch.tensor(1.0))

    def forward(self, x):
        return self.forward_stage2(*self.forward_stage1(x))

    def forward_stage1(self, x):
        h = torch.tanh(self.a(x))
        return (h, h)

    def forward_stage2(self, h1, h2):
        return self.b(0.5 * (h1 + h2)) * self.s

    def stage1_parameters(self):
        return self.a.parameters()


def _loss(o, t):
    return (o - t).pow(2).mean()


def _worker(rank, world, port, q, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip import checkpoint
    from adnm_hip.trainer import FlatTrainer

    def trainer(model, rd, ov):
        return FlatTrainer(model, _loss, lr=1e-2, eps=1e-9, weight_decay=1e-2, max_norm=0.5, use_graph=False, fused=False, reduce_dtype=rd,
                           overlap=ov)
    out = {}
    for ci, (rd, ov) in enumerate(CONFIGS):
        torch.manual_seed(100 + rank)
        data = [(torch.randn(5, 7), torch.randn(5, 3)) for _ in range(4)]
        model = Toy()
        tr = trainer(model, rd, ov)
        for x, t in data:
            tr.step(x, t)
        whole = {"params": [p.detach().numpy().copy() for p in model.parameters()], "m": tr.state_dict()}
        tr.close()
        model = Toy()
        tr = trainer(model, rd, ov)
        for x, t in data[:2]:
            tr.step(x, t)
        path = os.path.join(tmp, f"state_{ci}_rank{rank}.pth")
        checkpoint.save_training_state(tr, path)
        tr.close()
        model = Toy(seed=7 + rank)          # other weights, and not the same on the two ranks: the file must bring everything
        tr = trainer(model, rd, ov)
        checkpoint.load_training_state(tr, path)
        for x, t in data[2:]:
            tr.step(x, t)
        assert tr.staged == ov and tr._steps == 4
        sd = tr.state_dict()
        same = all(torch.equal(sd["params"][n][k], whole["m"]["params"][n][k]) for n in sd["params"] for k in ("exp_avg", "exp_avg_sq"))
        out[ci] = {"whole": whole["params"], "resumed": [p.detach().numpy().copy() for p in model.parameters()], "moments_equal": same}
        tr.close()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_resume_bit_for_bit(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for ci, (rd, ov) in enumerate(CONFIGS):
        a, b, what = res[0][ci], res[1][ci], f"reduce_dtype={rd} overlap={ov}"
        assert a["moments_equal"] and b["moments_equal"], f"{what}: moments after the resumed steps differ from the uninterrupted run's"
        for i, (w, ra, rb) in enumerate(zip(a["whole"], a["resumed"], b["resumed"])):
            assert (ra == rb).all(), f"{what}: the resumed replicas diverged at parameter {i}"
            assert (ra == w).all(), f"{what}: parameter {i} after the resume differs from the uninterrupted run's"
        assert any((w != 0).any() for w in a["whole"])

#!/usr/bin/env python3
"""SHA-256 of FlatTrainer's flat_p / flat_g after four training steps of a small model: the bitwise fingerprint of the whole step, for
comparing two checkouts (each with its own built library) after a refactor that must not move a bit.
create_ADNMUNet(5, 20, 6, img_size=64), recipe.fill_parameters, recipe.radar_batch(2, 25, 64, name="side"), lr 1e-3, max_norm 0.025 — the
set-up of profiles/side_lane_removed.txt §1.  One process per configuration:   python tools/step_digest.py eager|graph f32|bf16|fp8"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
os.environ["ADNM_AUTO_DDP"] = "0"
import torch
from adnm_hip import ops, recipe
from adnm_hip.trainer import FlatTrainer
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

mode, prec = sys.argv[1], sys.argv[2]
dev = torch.device("cuda", 0)
ops.set_mfma_precision(prec)
model = recipe.fill_parameters(create_ADNMUNet(5, 20, 6, img_size=64)).to(dev).train()
trainer = FlatTrainer(model, enRainfallLoss(omega_t=0.57, alpha=0.25, gamma=0.).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2,
                      max_norm=0.025, use_graph=mode == "graph")
frames = recipe.radar_batch(2, 25, 64, name="side").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
trainer.prepare(x, tgt)
for _ in range(4):
    trainer.step(x, tgt, eager=mode == "eager")
torch.cuda.synchronize()
for name in ("flat_p", "flat_g"):
    print(f"{mode:5s} {prec:4s}  {name} {hashlib.sha256(getattr(trainer, name).detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()}", flush=True)

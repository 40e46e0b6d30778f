"""Generates the GroupNorm / long-interval (LAPS) fixtures under tests/golden/ by running the REFERENCE's own Python
(through oracle/ref_harness.py), with the schemas of oracle/make_golden.py: module cases with InstanceNorm=False, the whole
create_ADNMUNet(5, 3, 60) model (GroupNorm, kernel [5,3,3], refine_dim [32,32,16,16]) and its state_dict manifest.

Needs the reference tree (ADNM_REFERENCE_ROOT); the fixtures are data only.  Run:  python tools/make_golden_groupnorm.py [--only REGEX]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))

import make_golden as G  # noqa: E402
import ref_harness as H  # noqa: E402
from adnm_hip import recipe  # noqa: E402


def build_laps(img_size, channels=5, out_channels=3):
    """The reference factory's hyper-parameters for frame_interval >= 120 / input_frames (ADNMUNet.py:906-940) at a chosen img_size.
    As in ref_harness.build_visionmamba, the decoder's literal 256 x 256 view is generalised by handing that one call a tensor
    subclass; the reference file is untouched."""
    A = H.load_reference().ADNMUNet
    model = A.VisionMamba(
        img_size=img_size, depth=[1, 1, 1], refine_depth=[1, 1, 1, 1], refine_headdim=[4, 4, 4, 4],
        refine_dim=[32, 32, 32, 32] if out_channels > 5 else [32, 32, 16, 16],
        embed_dim=[32, 64, 128, 256, 512, 1024], headdim=4, channels=channels, out_channels=out_channels,
        ssm_cfg=None, norm_epsilon=1e-6, initializer_cfg=None, kernel=[5, 3, 3], ratio=[2, 2, 2, 2, 2, 2],
        wt_levels=[3, 2, 1], out_expand=2, InstanceNorm=False)
    if img_size != 256:
        class SizedView(torch.Tensor):
            def view(self, *shape):
                if len(shape) == 4 and tuple(shape[1:3]) == (256, 256):
                    shape = (shape[0], img_size, img_size, shape[3])
                return super().view(*shape).as_subclass(torch.Tensor)

        model.decoder.decoder6.register_forward_hook(lambda m, i, o: o.as_subclass(SizedView))
    return model


def manifest():
    if not G.wanted("state_dict_manifest_laps"):
        return
    model = build_laps(64)
    consts = {}
    for k, v in model.state_dict().items():
        f = v.double().flatten()
        consts[k] = float(f[0]) if bool((f == f[0]).all()) else None
    recipe.fill_parameters(model)
    trainable = {k: p.requires_grad for k, p in model.named_parameters()}
    out = {k: {"shape": list(v.shape), "const": consts[k], "trainable": bool(trainable[k]),
               "sum": float(v.double().sum()), "abs": float(v.double().abs().sum())}
           for k, v in model.state_dict().items()}
    with open(os.path.join(G.OUT, "state_dict_manifest_laps.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"state_dict_manifest_laps: {len(out)} keys")


def main():
    U = H.load_reference().model_untils
    T = recipe.tensor
    G.module_case("gn_patch_embed_5_16", U.PatchEmbed(img_size=16, patch_size=2, in_channels=5, embed_dim=16, kernel=5, wt_levels=3,
                                                      InstanceNorm=False),
                  {"x": T("gpe.x", (2, 256, 5), positive=True)}, call=lambda mod, x: mod(x), grad_inputs=("x",))
    G.module_case("gn_wtlayer_16_24", U.WTLayer(16, 24, kernel=5, wt_levels=2, InstanceNorm=False), {"x": T("gwl.x", (2, 144, 16))},
                  call=lambda mod, x: mod(x), grad_inputs=("x",))
    # if_res: GroupNorm(8, 32), 4 channels per group; 3-wide wavelet kernels as the long-interval recipe's decoder
    G.module_case("gn_wtlayer_res_32_16", U.WTLayer(32, 16, kernel=3, wt_levels=1, if_res=True, InstanceNorm=False),
                  {"x": T("gwl2.x", (1, 64, 16)), "r": T("gwl2.r", (1, 64, 16)), "f": T("gwl2.f", (1, 64, 16))},
                  call=lambda mod, x, r, f: mod(x, residual=r, features=f), grad_inputs=("x", "r"))
    G.module_case("gn_e2d_16", U.EncoderToDecoder(embed_dim=16, InstanceNorm=False),
                  {"x": T("ge2d.x", (2, 64, 16)), "res": T("ge2d.r", (2, 64, 16))},
                  call=lambda mod, x, res: mod(x, res), grad_inputs=("x", "res"))
    G.module_case("gn_outproj_16_3", U.OutProj(num_frames=3, embed_dim=16, img_size=[16, 16], wt_levels=3, out_expand=2, InstanceNorm=False),
                  {"x": T("gop.x", (2, 256, 16)), "res": T("gop.r", (2, 16, 16), positive=True)},
                  call=lambda mod, x, res: mod(x, res), grad_inputs=("x",))
    manifest()
    # make_golden.whole_model_case builds its model through ref_harness.build_visionmamba: point that name at the long-interval
    # builder for these calls, so the schema (taps, samples, gradient norms / probes, the clipped AdamW step) is the same code
    saved, H.build_visionmamba = H.build_visionmamba, build_laps
    try:
        G.whole_model_case("laps_64_b2", 64, 2, radar="laps64", cin=5, cout=3, full_out=True, deltas=True)
        G.whole_model_case("laps_128_b1", 128, 1, radar="laps128", cin=5, cout=3, deltas=True)
        G.whole_model_case("laps_256_b1", 256, 1, radar="laps256", cin=5, cout=3, deltas=True)
    finally:
        H.build_visionmamba = saved


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="regex: regenerate only the fixtures whose name matches")
    G.ONLY = ap.parse_args().only
    main()

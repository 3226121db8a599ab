#!/usr/bin/env python
"""Produce the augmented prompt embedding that the SD experiment reads as validation_prompts[0] under using_augmented_prompt
(delete_sd.py:175-177, :235-241, :938) -- the reference makes it with LocalStableDiffusionPipeline.aug_prompt
(data/src/local_sd_pipeline.py:474-663) and ships no script for it:

    <out>.pt        the optimised embedding, [1, 77, X] f32
    <out>.json      the per-iteration noise norms (and, with --token-grads, the per-token gradient norms of the ORIGINAL prompt)

    python tools/make_aug_prompt.py --out aug_prompt.pt [--prompt "..." | --prompt-embeds x.pt] [--n 4] [--steps 50] [--iters 10]
                                    [--lr 0.1] [--target-step 0] [--target-loss L] [--optim-epsilon E] [--alpha 0.5] [--token-grads]
                                    [--allow-random-init] [--unet-json unet.json] [--config-name delete_sd] [key=value ...]

The prompt defaults to validation_prompts[0].  Needs the checkpoint directory (pretrained_model_name_or_path with unet/, and
text_encoder/ + tokenizer/ unless --prompt-embeds is given); --allow-random-init gives loudly announced stand-ins (random-init
weights of the configured architecture -- --unet-json: a JSON object of UNet2DConditionConfig fields --, synthetic embeddings)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-name", default="delete_sd")
    ap.add_argument("--config-path", default=os.path.join(ROOT, "config"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--prompt", default=None)
    ap.add_argument("--prompt-embeds", default=None)
    ap.add_argument("--n", type=int, default=4, help="num_images_per_prompt")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--target-step", type=int, default=0)
    ap.add_argument("--target-loss", type=float, default=None)
    ap.add_argument("--optim-epsilon", type=float, default=None)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--token-grads", action="store_true")
    ap.add_argument("--allow-random-init", action="store_true")
    ap.add_argument("--unet-json", default=None)
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args(argv)
    import torch
    from siss_amd import hydra_lite
    from siss_amd.prompt_aug import save_aug_prompt
    from siss_amd.tasks import DeleteSD
    over = list(a.overrides) + (["allow_random_init=true", "allow_synthetic=true"] if a.allow_random_init else [])
    cfg = hydra_lite.compose(a.config_name, a.config_path, over)
    if a.unet_json:
        with open(a.unet_json) as f:
            cfg.unet = json.load(f)
    task = DeleteSD(cfg)
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    unet = task.load_unet(device)
    sampler = task._validation_pipeline(unet, device)
    vp = cfg.get("validation_prompts")
    e = task._prompt_embedding(a.prompt_embeds or a.prompt or (vp[0] if vp else None), device)
    g = torch.Generator(device=device).manual_seed(task.seed())
    kw = dict(prompt_embeds=e, negative_prompt_embeds=task._negative_embeds, num_inference_steps=a.steps, guidance_scale=a.guidance,
              num_images_per_prompt=a.n, target_steps=[a.target_step])
    z = torch.randn((a.n, unet.config.in_channels, unet.config.sample_size, unet.config.sample_size), generator=g, device=device)
    tok = sampler.get_text_cond_grad(latents=z, **kw) if a.token_grads else None
    out, trace = sampler.aug_prompt(latents=z, lr=a.lr, optim_iters=a.iters, target_loss=a.target_loss, optim_epsilon=a.optim_epsilon,
                                    alpha=a.alpha, return_trace=True, **kw)
    path, side = save_aug_prompt(a.out, out, trace, tok)
    nn = trace["noise_norm"]
    print(f"{trace['iterations']} updates at step {trace['step']} (t = {trace['timestep']}): noise norm {nn[0]:.6g} -> {nn[-1]:.6g}"
          f"{' (stopped at target_loss)' if trace['stopped_early'] else ''}; wrote {path}, {side}")
    return path, side


if __name__ == "__main__":
    main()

"""Close the unpinned seams with a real checkpoint in minutes (CPU only; needs torch + safetensors, nothing from the reference).

Three pieces of the path rest on third-party code that is absent from the reference checkout and from the build image
(SURVEY.md 8c): SwissArmyTransformer 0.4.12's transformer internals (q|k|v order of `query_key_value`, biases,
`layernorm_epsilon`, `final_layernorm`) and vector-quantize-pytorch's codebook lookup.  This repo restates them from the
reference's call sites; no test here can falsify that restatement without the released weights.  Given the released tree

    python tools/verify_real_checkpoint.py --ckpt /path/to/ckpts/LanDiff            (layout: the reference's ckpts/README.md)

this script
  A. loads every component exactly as the product does (landiff_amd.weights.load_diffusion_states / load_llm_state) and audits
     keys + shapes against the specs the runners pack from (dit_spec, tokenizer_spec, upsampler_spec, vae_spec, llm_spec);
     the sat-owned keys are listed separately, with their bias presence;
  B. tests the `query_key_value` layout on trained weights: for each candidate layout it splits W into per-head q / k blocks
     and compares || Wq_h Wk_h^T ||_F of matching heads with mismatched heads -- trained attention couples a head's q and k
     projections, so the right layout has a same-head / cross-head ratio clearly above 1, wrong ones sit near 1
     (candidates: thirds with v first / middle / last, and the per-head interleaved [h][q,k,v][hd] form);
  C. measures what `layernorm_epsilon` = 1e-5 vs 1e-6 can change: the variance range of the real first-layer input rows
     (patch embedding of a N(0,1) latent + the checkpoint's position table) and the relative output difference of
     input_layernorm under the two values, next to the bf16 rounding step -- if the difference is below it, the choice cannot
     be observed in the product's arithmetic;
  D. checks the VQ codebook: shapes of `_codebook.embed` / `project_out`, whether every code is its own nearest code under the
     Euclidean rule the product uses, and whether the rows are unit-norm (a cosine-similarity codebook would need another rule).
  E. (--theia FILE_OR_DIR, or $LANDIFF_THEIA_CKPT / a local HF-cache snapshot when the flag is given without a value) audits the
     Theia checkpoint against the transformers 4.x ViTModel layout landiff_amd.theia reads (backbone.model.embeddings.*,
     encoder.layer.{i}.attention.attention.{query,key,value}, .attention.output.dense, .intermediate.dense, .output.dense,
     .layernorm_{before,after}, layernorm) at DeiT-base shapes, lists the key groups it ignores (translator.*, pooler.*), and
     loads it through load_theia_state.
Exit status 1 when a key or shape does not match (A, E); B-D print verdicts for a human.  `--config config0|tiny` checks a synthetic
tree written by landiff_amd.weights.save_checkpoint_tree (what tests/test_cabi_and_host.py does).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SAT_OWNED = ("input_layernorm", "post_attention_layernorm", "attention.query_key_value", "attention.dense",
             "mlp.dense_h_to_4h", "mlp.dense_4h_to_h", "transformer.final_layernorm")


def audit(name: str, sd: dict, spec) -> bool:
    want = {k: tuple(shape) for k, shape, _ in spec}
    missing = [k for k in want if k not in sd]
    wrong = [(k, tuple(sd[k].shape), want[k]) for k in want if k in sd and tuple(sd[k].shape) != want[k]]
    extra = [k for k in sd if k not in want]
    print(f"[A] {name}: {len(want)} keys expected, {len(want) - len(missing)} present, {len(wrong)} shape mismatches, {len(extra)} keys the runner does not use")
    for k in missing[:12]:
        print(f"      MISSING  {k} {want[k]}")
    for k, got, exp in wrong[:12]:
        print(f"      SHAPE    {k}: checkpoint {got}, expected {exp}")
    if extra[:6]:
        print(f"      unused   {extra[:6]}{' ...' if len(extra) > 6 else ''}")
    return not missing and not wrong


def sat_keys(sd: dict, layers: int):
    rows = {}
    for k, v in sd.items():
        for s in SAT_OWNED:
            if s in k:
                rows.setdefault(s, []).append((k, tuple(v.shape)))
    print("[A] sat-owned parameters (restated, not pinned) -- first instance of each, bias presence over all layers:")
    for s, items in rows.items():
        w = [i for i in items if i[0].endswith(".weight")]
        b = [i for i in items if i[0].endswith(".bias")]
        print(f"      {s:34s} weight {w[0][1] if w else None} x{len(w)}, bias {'present x%d' % len(b) if b else 'ABSENT'}")
    if "transformer.final_layernorm" not in rows:
        print("      transformer.final_layernorm ABSENT: the product applies it before FinalLayerMixin.final_forward (SURVEY 8c) -- check")


def qkv_layout(sd: dict, cfg, layer: int):
    w = sd[f"transformer.layers.{layer}.attention.query_key_value.weight"].float()
    d, H, hd = cfg.hidden, cfg.heads, cfg.head_dim
    assert tuple(w.shape) == (3 * d, d), w.shape
    thirds = [w[i * d:(i + 1) * d].view(H, hd, d) for i in range(3)]
    inter = w.view(H, 3, hd, d)

    def ratio(q, k):                                    # [H, hd, d] each
        m = torch.einsum("hid,gjd->hgij", q, k).flatten(2).norm(dim=2)          # [H, H] Frobenius norms of Wq_h Wk_g^T
        same = m.diagonal().mean().item()
        cross = (m.sum() - m.diagonal().sum()).item() / (H * H - H)
        return same / cross
    cands = {"thirds, v last  [q|k|v] (the product's assumption)": ratio(thirds[0], thirds[1]),
             "thirds, v middle [q|v|k]": ratio(thirds[0], thirds[2]),
             "thirds, v first  [v|q|k]": ratio(thirds[1], thirds[2]),
             "per-head interleaved [h][q,k,v][hd]": ratio(inter[:, 0], inter[:, 1])}
    best = max(cands, key=cands.get)
    print(f"[B] layer {layer}: same-head / cross-head coupling of the q and k projections per candidate layout")
    for n, r in cands.items():
        print(f"      {r:7.3f}  {n}")
    if max(cands.values()) < 1.15:
        print("      -> undecidable on these weights (all ratios ~ 1: random / synthetic checkpoint?)")
        return None
    ok = best.startswith("thirds, v last")
    print(f"      -> {'CONFIRMS' if ok else 'CONTRADICTS'} the product's layout: best = {best}")
    return ok


def ln_epsilon(sd: dict, cfg):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, cfg.latent_frames, cfg.in_channels, cfg.latent_h, cfg.latent_w, generator=g)
    p = cfg.patch
    w, b = sd["mixins.patch_embed.proj.weight"].float(), sd["mixins.patch_embed.proj.bias"].float()
    e = F.conv2d(x[0], w, b, stride=p).flatten(2).transpose(1, 2).reshape(-1, cfg.hidden)            # [T*h*w, d]
    pos = sd["mixins.pos_embed.pos_embedding"].float()[0, cfg.text_len:cfg.text_len + e.shape[0]]
    h = e + pos
    var = h.var(dim=1, unbiased=False)
    lw, lb = sd["transformer.layers.0.input_layernorm.weight"].float(), sd["transformer.layers.0.input_layernorm.bias"].float()
    a = F.layer_norm(h, (cfg.hidden,), lw, lb, 1e-5)
    c = F.layer_norm(h, (cfg.hidden,), lw, lb, 1e-6)
    rel = ((a - c).abs().max() / c.abs().max()).item()
    print(f"[C] first-layer input rows (patch embedding of a N(0,1) latent + position table): variance min {var.min():.3e}, median {var.median():.3e}")
    print(f"      input_layernorm with eps 1e-5 vs 1e-6: max relative output difference {rel:.2e}; one bf16 rounding step is 3.9e-03")
    print("      -> " + ("the two values are indistinguishable in bf16 arithmetic at this layer" if rel < 1e-3 else
                         "the value IS observable: compare one real layer output of the reference under both and set DiTConfig.block_ln_eps"))


def vq_check(sd: dict, tc):
    emb = sd["quantizer._codebook.embed"].float()
    print(f"[D] quantizer._codebook.embed {tuple(emb.shape)}; project_out "
          f"{tuple(sd['quantizer.project_out.weight'].shape) if 'quantizer.project_out.weight' in sd else 'ABSENT (codebook_dim == dim)'}")
    e = emb[0]
    d2 = (e * e).sum(1)[:, None] - 2 * e @ e.t() + (e * e).sum(1)[None]
    self_nearest = bool((d2.argmin(1) == torch.arange(e.shape[0])).all())
    norms = e.norm(dim=1)
    print(f"      every code is its own nearest code (Euclidean): {self_nearest}; row norms min {norms.min():.3f} max {norms.max():.3f}"
          + ("  <- unit-norm rows: a cosine-similarity codebook? the product searches by Euclidean distance" if (norms - 1).abs().max() < 1e-3 else ""))


def theia_spec(width: int = 768, layers: int = 12, pos: int = 197):
    """(key, shape, None) of the DeiT-base backbone below backbone.model. (landiff_amd.theia.theia_keys)."""
    from landiff_amd.theia import theia_keys
    fixed = {"embeddings.cls_token": (1, 1, width), "embeddings.position_embeddings": (1, pos, width),
             "embeddings.patch_embeddings.projection.weight": (width, 3, 16, 16)}
    out = []
    for k in theia_keys(layers):
        if k in fixed:
            sh = fixed[k]
        elif k.endswith("intermediate.dense.weight"):
            sh = (4 * width, width)
        elif k.endswith("intermediate.dense.bias"):
            sh = (4 * width,)
        elif k.endswith(".output.dense.weight") and ".attention." not in k:
            sh = (width, 4 * width)
        elif k.endswith(".weight") and "layernorm" not in k:
            sh = (width, width)
        else:
            sh = (width,)
        out.append(("backbone.model." + k, sh, None))
    return out


def theia_check(path: str | None) -> bool:
    from safetensors.torch import load_file
    from landiff_amd.theia import load_theia_state, resolve_theia_path, theia_dims
    f = resolve_theia_path(path)
    sd = load_file(f)
    groups = {}
    for k in sd:
        if not k.startswith("backbone.model.") or k.startswith("backbone.model.pooler."):
            g = ".".join(k.split(".")[:3 if k.startswith("backbone.") else 1])
            groups[g] = groups.get(g, 0) + 1
    print(f"[E] Theia {f}: {len(sd)} tensors; ignored groups {dict(sorted(groups.items()))}")
    ok = audit("Theia backbone (DeiT-base, transformers 4.x ViTModel names)", {k: v for k, v in sd.items()}, theia_spec())
    if ok:
        print(f"      load_theia_state: {theia_dims(load_theia_state(f))}")
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ckpt", required=True, help="the checkpoint root (ckpts/LanDiff of the reference layout)")
    ap.add_argument("--config", default="full", choices=["full", "config0", "tiny"])
    ap.add_argument("--theia", nargs="?", const="", default=None,
                    help="also audit the Theia checkpoint (a model.safetensors or its directory; without a value: "
                         "$LANDIFF_THEIA_CKPT, then a local Hugging Face cache snapshot)")
    args = ap.parse_args()
    from landiff_amd.config import PipelineConfig
    from landiff_amd.weights import (CKPT_FILES, dit_spec, llm_spec, load_diffusion_states, load_llm_state, tokenizer_spec, upsampler_spec, vae_spec)
    cfg = {"full": PipelineConfig.full, "config0": PipelineConfig.config0, "tiny": lambda: PipelineConfig.tiny(2)}[args.config]().check()
    root = args.ckpt
    st = load_diffusion_states(os.path.join(root, "diffusion"), root, tokenizer_ckpt=os.path.join(root, CKPT_FILES["tokenizer"]))
    ok = True
    ok &= audit("main DiT (CogVideoX base + control checkpoint on top)", st["dit_main"], dit_spec(cfg.dit, False))
    ok &= audit("control DiT", st["dit_control"], dit_spec(cfg.dit, True))
    ok &= audit("tokenizer (TiTok decoder + VQ)", st["tok"], tokenizer_spec(cfg.tok))
    ok &= audit("conv upsampler + conv_out", st["ups"], upsampler_spec(cfg.ups))
    ok &= audit("3D-VAE decoder", st["vae"], vae_spec(cfg.vae))
    llm_path = os.path.join(root, CKPT_FILES["llm"])
    if os.path.exists(llm_path):
        ok &= audit("AR language model", load_llm_state(llm_path), llm_spec(cfg.llm))
    else:
        print(f"[A] AR language model: {llm_path} not found, skipped")
    sat_keys(st["dit_main"], cfg.dit.layers_main)
    verdicts = [qkv_layout(st["dit_main"], cfg.dit, i) for i in sorted({0, cfg.dit.layers_main // 2, cfg.dit.layers_main - 1})]
    ln_epsilon(st["dit_main"], cfg.dit)
    vq_check(st["tok"], cfg.tok)
    if args.theia is not None:
        ok &= theia_check(args.theia or None)
    print("SUMMARY: keys/shapes " + ("OK" if ok else "MISMATCH") + "; qkv layout " +
          ("undecidable" if all(v is None for v in verdicts) else "confirmed" if all(v in (True, None) for v in verdicts) else "CONTRADICTED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

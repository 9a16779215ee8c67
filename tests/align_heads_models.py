"""Models and inputs shared by the per-head alignment tests (tests/test_align_heads_refs.py, tests/test_gpu_align_heads.py and
tests/golden/gen_golden_align_heads.py): the tiny geometry (2 decoder layers x 2 heads), a 3-layer x 4-head geometry built the
same way (d_model 256), and a wide one (4 decoder layers x 20 heads, d_model 1280) whose capture buffer is larger than the
context's own.  Weights are the "aligned" synthetic ones: the designed alignment heads (synthetic.alignment_heads) are peaked
and move through the audio, every other head is a seeded random one."""
from __future__ import annotations

import numpy as np

from crisperwhisper_amd import synthetic as syn


def geometry(name):
    v = syn.SynthVocab(n_extra=0)
    if name == "tiny":
        return syn.tiny_geometry()
    if name == "mid":
        return syn.Geometry(d_model=256, heads=4, ffn=512, enc_layers=2, dec_layers=3, n_mels=128, vocab=v.size), v
    if name == "wide":
        return syn.Geometry(d_model=1280, heads=20, ffn=1280, enc_layers=1, dec_layers=4, n_mels=128, vocab=v.size), v
    raise ValueError(name)


def weights(g, seed=0):
    return {n: syn.weight_tensor(g, n, shape, seed, "aligned") for n, shape in syn.weight_shapes(g).items()}


def all_heads(g):
    return [[l, h] for l in range(g.dec_layers) for h in range(g.heads)]


def setup(name, seed=0):
    g, v = geometry(name)
    return g, v, weights(g, seed), syn.model_spec(g, v, 3)


def rows(v, lengths, seed):
    """Whole decoder inputs of the given lengths: 3 init tokens, byte-level text with a space every few tokens, eos."""
    rng = np.random.default_rng(seed)
    init = [v.sot, v.lang_id("en"), v.transcribe]
    out = []
    for n in lengths:
        text = rng.integers(ord("a"), ord("z") + 1, n - 4)
        text[::4] = ord(" ")
        out.append(np.concatenate([init, text, [v.eos]]).astype(np.int64))
    return out


def hf_model(name, seed=0):
    """The same model as a transformers WhisperForConditionalGeneration (eager attention), its tokenizer and feature extractor:
    (g, v, W, spec, model, tokenizer, feature_extractor).  Only the reference side of the tests uses it."""
    import torch
    from tests.golden import hf_synth as H
    g, v, W, spec = setup(name, seed)
    model = H.build_model(g, v, n_align=3)
    sd = {k: torch.from_numpy(x) for k, x in W.items()}
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    model.load_state_dict(sd, strict=True)
    model.config._attn_implementation = "eager"
    return g, v, W, spec, model, H.build_tokenizer(v), H.build_feature_extractor(g)

"""Which launches a decoder layer has: the (kernel, launches) list of Engine.time_decode_stages per configuration and row count,
pinned against tests/golden/decode_stage_tables.json.  The row counts are both sides of every threshold of the decode step's plan
(8 | 9: qkv_self and the short self-attention history, 16 | 17: one MFMA half tile against row groups, 32 | 33: the column-owning
cross out-projection, 64: the largest batch).  The fixture was recorded at commit c0e05c9, before decode_step was split into a plan and
one function per layer path; it is a record of what the step launched then, not of what it should launch: a change that moves a
launch on purpose re-records it (record() below) and says so."""
import json
import os

import numpy as np
import pytest

from crisperwhisper_amd import synthetic as syn
from crisperwhisper_amd.engine import Engine
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

FIXTURE = "decode_stage_tables.json"
ROWS = (1, 8, 9, 16, 17, 32, 33, 64)

# name -> (geometry, dtype, cross_kv_dtype, environment at creation)
CONFIGS = {
    "bf16": ("large", "bf16", None, {}),
    "f16": ("large", "f16", None, {}),
    "bf16_kv8": ("large", "bf16", "fp8", {}),
    "bf16_no_fuse6": ("large", "bf16", None, {"CW_NO_FUSE6": "1"}),
    "bf16_no_fuse_rows": ("large", "bf16", None, {"CW_NO_FUSE_ROWS": "1"}),
    "bf16_no_own_cols": ("large", "bf16", None, {"CW_NO_OWN_COLS": "1"}),
    "bf16_no_qkv_self": ("large", "bf16", None, {"CW_NO_QKV_SELF": "1"}),
    "bf16_no_wpack": ("large", "bf16", None, {"CW_NO_WPACK": "1"}),
    "bf16_no_ln_fold": ("large", "bf16", None, {"CW_NO_LN_FOLD": "1"}),
    "bf16_kv8_no_fuse_rows8": ("large", "bf16", "fp8", {"CW_NO_FUSE_ROWS8": "1"}),
    "f32_tiny": ("tiny", "f32", None, {}),
}
# the measured-and-rejected variants (-DCW_EXPERIMENTS builds): name -> (environment at creation, rows)
EXPERIMENTS = {
    "fuse_mlp": ({"CW_FUSE_MLP": "1"}, 8),
    "mlp_pair": ({"CW_MLP_PAIR": "1"}, 8),
    "declayer": ({"CW_DECLAYER": "1"}, 8),
    "mlp_chain": ({"CW_MLP_CHAIN": "1"}, 8),
    "rows_ln": ({"CW_ROWS_LN": "1"}, 64),
    "skinny1": ({"CW_SKINNY": "1"}, 64),
    "skinny2": ({"CW_SKINNY": "2"}, 64),
}

_MODELS = {}


def _model(geometry):
    """(spec, weights) of a geometry, made once per process."""
    if geometry not in _MODELS:
        if geometry == "tiny":
            g, v, W, spec = Hh.tiny_setup()
        else:           # large-v3 shapes on a 2 + 2-layer stack: own, qkv_self residency and the D <= 1280 limits need these sizes
            g, v = syn.large_v3_geometry()
            g.enc_layers = g.dec_layers = 2
            spec = syn.model_spec(g, v, n_align=15)
            spec.alignment_heads = [[l, h] for l in range(2) for h in (0, 3, 7, 19)]
            W = syn.random_weights(g, seed=9)
        _MODELS[geometry] = (spec, W)
    return _MODELS[geometry]


def stage_tables(geometry, dtype, kv, env, rows):
    """{str(nb): [[kernel name, launches], ...]} of one engine, 64 windows encoded (their content is irrelevant)."""
    spec, W = _model(geometry)
    os.environ.update(env)
    try:
        eng = Engine(spec, dtype=dtype, max_batch=64, cross_kv_dtype=kv)     # a context's switches are fixed at creation
    finally:
        for k in env:
            os.environ.pop(k, None)
    try:
        eng.load_state_dict(W)
        eng.set_features(np.random.default_rng(0).standard_normal((1, spec.n_mels, 3000)).astype(np.float32))
        eng.encode([0] * 64, [0] * 64, [3000] * 64)
        return {str(nb): [[st["kernel"], st["launches"]] for st in eng.time_decode_stages(nb, 1) if st["stage"] >= 0] for nb in rows}
    finally:
        eng.close()


def record(path=os.path.join(Hh.GOLD, FIXTURE)):
    """Writes the fixture from the library this process loads (the product library: CONFIGS; a -DCW_EXPERIMENTS build, through
    CW_LIB_PATH: EXPERIMENTS), keeping the entries it does not produce.  Never called by the tests."""
    table = json.load(open(path)) if os.path.exists(path) else {}
    if Hh.has_experiments():
        for name, (env, nb) in EXPERIMENTS.items():
            table["experiments_" + name] = stage_tables("large", "bf16", None, env, (nb,))
    else:
        for name, cfg in CONFIGS.items():
            table[name] = stage_tables(*cfg, ROWS)
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


def _check(got, want):
    for nb in want:
        print(nb, got[nb])
    assert got == want, {nb: (got[nb], want[nb]) for nb in want if got[nb] != want[nb]}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_decoder_layer_launch_table(name):
    _check(stage_tables(*CONFIGS[name], ROWS), Hh.gold_json(FIXTURE)[name])


@pytest.mark.parametrize("name", list(EXPERIMENTS))
def test_rejected_variant_launch_table(request, name):
    """The differential tests of the rejected variants compare a variant with the default path: they would still pass if a
    mis-routed switch ran the default path on both sides.  This pins that each switch reaches its own launches."""
    if not Hh.has_experiments():
        return Hh.run_in_child(request, Hh.experiments_env(), lambda p: True)
    env, nb = EXPERIMENTS[name]
    _check(stage_tables("large", "bf16", None, env, (nb,)), Hh.gold_json(FIXTURE)["experiments_" + name])

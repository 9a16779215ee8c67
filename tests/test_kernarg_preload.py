"""Kernel-argument preload of the <= 16-row decode step (DESIGN.md 6g'').

Descriptor check (no GPU): the kernels' leading plain arguments are placed in user SGPRs at dispatch only while they stay in front
of the first by-value struct and within 14 dwords; the kernel descriptor in the library's gfx950 code object records how many
dwords that is.  Reordering arguments would silently lose the preload -- the kernels would still compute the same.

Graph replay equals eager launch (GPU): preloaded arguments are baked into the graph nodes at capture, the one new runtime path."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from crisperwhisper_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel function -> dwords of its leading plain arguments (pointers: 2, 32-bit integers: 1), as the signatures in csrc/ declare them
LEADING_DWORDS = {
    "gemv2_bf16_kernel": 14,         # x, W, bias, aux | K, Kb, N, rows, cb_H, cb_plane
    "gemv_loop_kernel": 14,          # x, W, ln_g, ln_b, bias | Mb, K, N, grid_x
    "attn_cross_split_kernel": 14,   # Kp, Vp, pstats, qa, qw, qbias | dims, qb_off
    "qkv_self_kernel": 14,           # x, Wp, bias, sk, sv, pos | dims, cap
    "gemv_stack_kernel": 7,          # Wp, zero | zero_n4, dims, blocks12
    "sample_partial_kernel": 14,     # logits, ids_all, cfg, pos, last_ts_tok, mask | ldv, ids_stride
    "sample_kernel": 14,             # ids_all, cfg, pos, finished, last_ts_tok, partials | ids_stride, timestamp_begin
}
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _gfx950_code_objects(blob):
    """the gfx950 ELF images of every (uncompressed) clang offload bundle in the library's .hip_fatbin section"""
    out, at = [], blob.find(BUNDLE_MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(BUNDLE_MAGIC))
        o = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, o)
            triple = blob[o + 24:o + 24 + tlen]
            o += 24 + tlen
            if triple.endswith(b"gfx950") and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(BUNDLE_MAGIC, at + 1)
    return out


def _kernel_descriptors(elf):
    """{symbol without '.kd': the 64-byte kernel descriptor} of one ELF64 little-endian code object"""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr off size link info align entsize
    found = {}
    for s in secs:
        if s[1] != 2:                                      # SHT_SYMTAB
            continue
        stroff = secs[s[6]][4]
        for i in range(s[5] // 24):
            name_off, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, s[4] + i * 24)
            end = elf.index(b"\0", stroff + name_off)
            name = elf[stroff + name_off:end].decode()
            if not name.endswith(".kd") or shndx == 0 or shndx >= len(secs):
                continue
            sec = secs[shndx]
            at = sec[4] + (value - sec[3])
            found[name[:-3]] = elf[at:at + 64]
    return found


def _preload_length(kd):
    """KERNARG_PRELOAD_SPEC_LENGTH: bits 0..6 of the 16-bit field at byte 58 of the descriptor, behind KERNEL_CODE_PROPERTIES
    (dwords in user SGPRs)"""
    return struct.unpack_from("<H", kd, 58)[0] & 0x7F


@pytest.fixture(scope="module")
def descriptors():
    path = _native.LIB_PATH
    if not os.path.exists(path):
        pytest.skip(f"{path} is not built")
    blob = open(path, "rb").read()
    objs = _gfx950_code_objects(blob)
    if not objs:
        pytest.skip("no uncompressed gfx950 code object in the library's offload bundles (a compressed bundle needs the LLVM tools)")
    kds = {}
    for elf in objs:
        kds.update(_kernel_descriptors(elf))
    return kds


@pytest.mark.parametrize("kernel", sorted(LEADING_DWORDS))
def test_descriptor_preload_length(descriptors, kernel):
    """every instantiation of the kernel, in both dtype builds (namespaces cw_bf16, cw_f16)"""
    mine = {}
    for ns in ("cw_bf16", "cw_f16"):
        head = f"_ZN{len(ns)}{ns}{len(kernel)}{kernel}I"          # Itanium mangling of <ns>::<kernel><template arguments ...>
        here = {n: kd for n, kd in descriptors.items() if n.startswith(head)}
        assert here, f"{ns}::{kernel}: no instantiation in the library"
        mine.update(here)
    wrong = {n: _preload_length(kd) for n, kd in mine.items() if _preload_length(kd) != LEADING_DWORDS[kernel]}
    assert not wrong, f"{kernel}: kernarg preload length != {LEADING_DWORDS[kernel]} dwords: {wrong}"


def test_descriptor_parser_reads_the_field(descriptors):
    """translation units built without the flag (the encoder's, the front end's) carry length 0"""
    assert len(descriptors) > 100 and any(_preload_length(kd) == 0 for kd in descriptors.values())


# ---------------------------------------------------------------------------------------------------
# graph replay == eager launch
# ---------------------------------------------------------------------------------------------------
DTYPES = ("bf16", "f16")
ROWS = (1, 5, 8, 9, 16)
N_NEW = 12


def _worker(out_path):
    """Child process (graph or CW_NO_GRAPH=1, fixed at the first launch): per (dtype, rows) one engine, N_NEW free-running tokens
    over the tiny model; token ids, the logits of every step, alignment rows and token timestamps into one .npz"""
    from crisperwhisper_amd import synthetic as syn
    from crisperwhisper_amd.engine import Engine
    from tests import helpers as Hh
    g, v, W, spec = Hh.tiny_setup()
    x = syn.synth_audio(0, 30 * 16000, "mixed")
    prompt1 = [v.sot, spec.lang_to_id["<|en|>"], spec.task_to_id["transcribe"]]
    n_prompt, L = len(prompt1), len(prompt1) + N_NEW
    res = {}
    for dt in DTYPES:
        for nb in ROWS:
            eng = Engine(spec, dtype=dt, max_batch=16)
            eng.load_state_dict(W)
            eng.mel([x])
            seek = [60 * b for b in range(nb)]                        # every row its own window of the one clip
            frames = [2000 - 50 * b for b in range(nb)]
            eng.encode([0] * nb, seek, frames)
            prompt = np.tile(np.asarray(prompt1, np.int32), (nb, 1))
            seqs, lens, _ = eng.decode(prompt, max_length=L, min_new_tokens=N_NEW)
            key = f"{dt}_{nb}"
            res[key + "_ids"] = seqs[:, :L].copy()
            res[key + "_lens"] = lens.copy()
            res[key + "_align"] = eng.alignment(nb, L - 1)
            res[key + "_ts"] = eng.token_timestamps(nb, L - 1, n_prompt, frames)
            if os.environ.get("CW_NO_GRAPH"):
                cap = eng.capture_logits(nb, N_NEW)                    # capturing takes the launch-per-kernel path anyway
                eng.decode(prompt, max_length=L, min_new_tokens=N_NEW)
                res[key + "_logits"] = cap.copy()
                eng.stop_capture()
            else:
                # a capture buffer would take the engine off the graph: the logits of step s are what the graph leaves behind
                # when the same decode stops after s + 1 tokens (every call replays the captured step with moving positions)
                steps = []
                for s in range(N_NEW):
                    eng.decode(prompt, max_length=n_prompt + s + 1, min_new_tokens=N_NEW)
                    steps.append(eng.last_logits(nb))
                res[key + "_logits"] = np.stack(steps)
            eng.close()
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def replay_runs(tmp_path_factory):
    """two fresh child processes, one per launch mode; each runs every (dtype, rows) case once"""
    tmp = tmp_path_factory.mktemp("kpl")
    out = {}
    for mode, no_graph in (("graph", None), ("eager", "1")):
        env = dict(os.environ)
        env.pop("CW_NO_GRAPH", None)
        if no_graph:
            env["CW_NO_GRAPH"] = no_graph
        path = str(tmp / f"{mode}.npz")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
            "-c", f"import sys; sys.path.insert(0, {ROOT!r}); from tests import test_kernarg_preload as t; t._worker({path!r})"]
        p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        if p.returncode < 0 or p.returncode > 128:
            pytest.exit(f"the {mode} child of test_kernarg_preload died (rc={p.returncode}): {p.stderr[-3000:]}\n"
                        "stopping the session: nothing more runs on a device that may be faulted", returncode=1)
        assert p.returncode == 0, f"{mode} child failed (rc={p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
        out[mode] = dict(np.load(path))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_equals_eager_launch(replay_runs, dtype, rows):
    g, e = replay_runs["graph"], replay_runs["eager"]
    key = f"{dtype}_{rows}"
    assert g[key + "_lens"].tolist() == [3 + N_NEW] * rows, f"the rows did not run freely for {N_NEW} tokens"
    for what in ("ids", "lens", "logits", "align", "ts"):
        a, b = g[f"{key}_{what}"], e[f"{key}_{what}"]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), f"{what}: graph replay differs from eager launch ({int((a != b).sum())} elements)"
    assert np.isfinite(g[key + "_logits"]).all()

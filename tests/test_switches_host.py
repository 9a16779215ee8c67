"""The A/B switch table (csrc/switches.def) on the host: csrc/switches.cpp and tests/native/switches_dump.cpp under
AddressSanitizer + UndefinedBehaviorSanitizer (plain g++, no HIP).  What every field parses to, and what the launcher options of
cw_test_set_option do to the process table, is held to tests/golden/switches_env.json, which was recorded from the hand-written
parser the table replaced (the fixture names the commit)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "switches_env.json")))
ENV_WANT = {c["name"]: c for c in GOLDEN["environment"]}

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("switches") / "switches_dump"
    src = [os.path.join(ROOT, "tests", "native", "switches_dump.cpp"), os.path.join(ROOT, "crisperwhisper_amd", "csrc", "switches.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", *src, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in (r.stderr or ""):
        pytest.skip("toolchain without sanitizer runtimes: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]

    def run(env, *pairs):
        base = {k: v for k, v in os.environ.items() if not k.startswith("CW_")}
        r = subprocess.run([str(exe), *pairs], capture_output=True, text=True, timeout=60,
                           env=dict(base, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **env))
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
        blocks = []
        for ln in r.stdout.split("\n"):
            if ln.startswith("# "):
                blocks.append((ln[2:], {}))
            elif ln:
                k, v = ln.split("=")
                assert k not in blocks[-1][1], k
                blocks[-1][1][k] = int(v)
        return blocks
    return run


def test_table_has_every_field_once(driver):
    (_, got), = driver({})
    assert sorted(got) == sorted(ENV_WANT["empty"]["want"]) and len(got) == 61


@pytest.mark.parametrize("name", list(ENV_WANT))
def test_environment_parses_as_before(driver, name):
    case = ENV_WANT[name]
    (head, got), = driver(case["env"])
    assert head == "environment"
    diff = {k: (got.get(k), v) for k, v in case["want"].items() if got.get(k) != v}
    assert not diff and len(got) == len(case["want"]), diff


@pytest.mark.parametrize("env,back", [({}, 0), ({"CW_MEL_VALU": "1"}, 1)])
def test_mel_valu_option_edits_its_field_alone_and_returns_to_the_environment(driver, env, back):
    """the option added after the fixture was recorded (tests/test_gpu_mel.py selects mel_kernel with it): 1 / 0 set the field, a
    negative value copies it back from the environment, nothing else moves"""
    blocks = driver(env, "mel_valu=1", "mel_valu=0", "mel_valu=-1")
    assert [h for h, _ in blocks[1:]] == ["mel_valu=1 ok", "mel_valu=0 ok", "mel_valu=-1 ok"]
    assert [g["mel_valu"] for _, g in blocks] == [back, 1, 0, back]
    for _, g in blocks[1:]:
        assert dict(g, mel_valu=back) == blocks[0][1]


@pytest.mark.parametrize("i", range(len(GOLDEN["options"])))
def test_options_edit_the_process_table(driver, i):
    case = GOLDEN["options"][i]
    env = ENV_WANT[case["env"]]
    blocks = driver(env["env"], *["%s=%d" % (s["option"], s["value"]) for s in case["steps"]])
    assert blocks[0][1] == env["want"] and len(blocks) == 1 + len(case["steps"])
    for s, (head, got) in zip(case["steps"], blocks[1:]):
        assert head == "%s=%d %s" % (s["option"], s["value"], "ok" if s["ok"] else "rejected")
        assert got == dict(env["want"], **s["differs"]), (head, {k: v for k, v in got.items() if env["want"][k] != v})

"""one_amd/csrc/host_stage_plan.h - which way HostStage::move sends a transfer of caller memory
(route, whole pages registered, partial pages and small transfers through the arena in pieces) and
where runHost cuts a host-buffer batch into chunks - is plain C++ without HIP: compiled with g++
under AddressSanitizer and UBSan into a stand-alone program (tests/cpp/host_stage_plan_test.cpp)
and held against a brute-force byte map of "this byte's page lies wholly inside the buffer", at
every page offset crossed with the lengths around every threshold, on random cases and on
buffers that sit back to back.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_stage_plan_on_the_host(tmp_path):
    prog = str(tmp_path / "host_stage_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "one_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "host_stage_plan_test.cpp"), "-o", prog],
                   check=True)
    assert subprocess.run([prog], capture_output=True).returncode == 2   # says so without its argument
    run = subprocess.run([prog, "4000"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    said = re.fullmatch(r"host stage plan ok: (\d+) transfer plans agreed with the brute-force rule, "
                        r"(\d+) chunk plans held\n", run.stdout)
    assert said, run.stdout + run.stderr
    # 4,096 offsets x 16 edge lengths x 16 settings, the random and the back-to-back cases
    assert int(said.group(1)) >= 4096 * 16 * 16 + 4000 * 4 and int(said.group(2)) >= 1000


def test_host_stage_takes_its_thresholds_from_the_plan():
    """host_stage.h defines no threshold of its own, and redgpu.cpp no chunk plan"""
    with open(os.path.join(ROOT, "one_amd", "csrc", "host_stage.h")) as f:
        text = f.read()
    assert '#include "host_stage_plan.h"' in text
    assert re.search(r"kBounceMax = kStageBounceMax;", text)
    assert re.search(r"kDirectFrom = kStageDirectFrom;", text)
    for name in ("host_stage.cpp", "redgpu.cpp"):
        with open(os.path.join(ROOT, "one_amd", "csrc", name)) as f:
            body = f.read()
        assert not re.search(r"chunkCuts\(const uint64_t", body), name
        assert "constexpr uintptr_t kPage" not in body and "constexpr size_t kPiece" not in body, name

"""CPU tier: the graded column split of the general matrix-core EQ kernel (csrc/mfma_plan.hpp: plan_columns_graded) as plain arithmetic."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graded_column_plan_properties(tmp_path):
    """tests/mfma_graded_plan_check.cpp, built by the host compiler with AddressSanitizer + UBSan (runtimes linked statically: the program runs
    directly, nothing is preloaded), over n in {1, 33, 4096, 131072, 1000003} x ntile in {1, 8, 9, 63, 64, 129, 257, 4096, 16385}, 64 rows per wave,
    1 / 512 / 1024 resident slots: start[0] = 0 and start[js] = ntile, strictly increasing boundaries that cover every tile once, non-increasing
    lengths behind the body, no chunk under the floor or off the stage length but the last, js <= 64, the uniform plan where the shape is too small;
    and the contract shape's 6 x 512 + 2 x 256 + 2 x 128 + 4 x 64 tiles."""
    exe = tmp_path / "mfma_graded_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "mfma_graded_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mfma_graded_plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]

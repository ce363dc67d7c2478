"""Child process of test_materials_at_the_resident_shape (tests/test_gpu_shading_synthetic.py).  The parent sets RTGGX_TRACE_WAVES, which the
library reads once per process: every trace launch of this process is a resident workgroup of that many waves with the tree tops in LDS,
the shape a frame has from RT_TINY_RAYS rays on -- which these small frames never reach by themselves, whatever
rtggx_debug_trace_residency pins (trace.hip launchTrace).  The materials family, every frame bit for bit and under the code rule."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import shading_cases as SC  # noqa: E402
import test_gpu_shading_synthetic as T  # noqa: E402

assert os.environ.get("RTGGX_TRACE_WAVES"), "the parent sets the size"
for case in SC.all_cases():
    if case.family == "materials":
        used = T.run_case(case)
        assert all(b > 0 for _, b in used.values()), case.name
print("resident shading ok")

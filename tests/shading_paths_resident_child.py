"""Child process of test_samples_and_depth_at_the_resident_shape (tests/test_gpu_shading_paths.py).  The parent sets RTGGX_TRACE_WAVES, which
the library reads once per process: every trace launch of this process -- every level of every sample -- is a resident workgroup of that
many waves with the tree tops in LDS (tests/shading_resident_child.py has the why).  Two samples of two levels in the black metallic room
and in the room whose walls reflect, every frame bit for bit and under the code rule."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import shading_cases as SC  # noqa: E402
import test_gpu_shading_paths as T  # noqa: E402

assert os.environ.get("RTGGX_TRACE_WAVES"), "the parent sets the size"
for name in T.RESIDENT_RUNS:
    used = T.run_path(SC.path_by_name(name))
    assert all(b > 0 for _, b in used.values()), name
print("resident paths ok")

"""Child process of test_a_pick_at_the_resident_shape (tests/test_gpu_shading_sampled.py).  The parent sets RTGGX_TRACE_WAVES, which the
library reads once per process: every trace launch of this process -- the any-hit traversal of the shadow rays among them -- is a resident
workgroup of that many waves with the tree tops in LDS.  One pick run, every frame bit for bit and under the stage check."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import shading_cases as SC  # noqa: E402
import test_gpu_shading_sampled as D  # noqa: E402
import test_shading_sampled_host as T  # noqa: E402

assert os.environ.get("RTGGX_TRACE_WAVES"), "the parent sets the size"
run = SC.sampled_by_name("pick_radii_75x53")
got, used = T.measure(run, D.run_device(run))
assert all(b > 0 for _, b in used.values()) and got["reach"] == T.recorded()["cases"][run.name]["reach"], run.name
print("resident sampled shading ok")

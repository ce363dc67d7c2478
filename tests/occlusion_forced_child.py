"""Child process of test_resident_workgroups_through_the_forced_size (tests/test_gpu_occlusion.py).  The parent sets RTGGX_TRACE_WAVES, which the
library reads once per process: every trace launch of this process, the any-hit ones included, is a resident workgroup of that many waves.
Two lists: 100 000 rays (two waves per bin) and 262 144 (a wave per bin)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import occlusion_cases as OC  # noqa: E402

assert os.environ.get("RTGGX_TRACE_WAVES"), "the parent sets the size"
ctx, o, rays = OC.long_list_context()
try:
    for n in (100000, 262144):
        OC.check_long_list(ctx, o, rays, n)
finally:
    ctx.close(); o.close()
print("resident lists ok")

// TEST INFRASTRUCTURE ONLY.  The one translation unit of the CPU restatements, built by tests/restatement.py with the oracle Makefile's flags
// into tests/_build/librestatement.so: the whole CPU oracle (oracle/orc_capi.cpp, through tests/recursion_ref.cpp) once, and beside its
// orc_ray_trace the entry points orc_ray_trace_depth (recursion_ref.cpp), orc_ray_trace_spp / _spp_f32 (spp_ref.cpp) and
// orc_ray_trace_sampleset (sampleset_ref.cpp; its functions carry _m in their names).  -ffp-contract=off -fno-fast-math keep each
// function's results independent of its neighbours; the host tests compare the layers bit for bit (tests/test_recursion_host.py,
// test_spp_host.py, test_sampleset_host.py).
#include "spp_ref.cpp"          // which includes recursion_ref.cpp, which includes ../oracle/orc_capi.cpp
#include "sampleset_ref.cpp"

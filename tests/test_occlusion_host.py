"""Occlusion queries, the part that needs no GPU: rtggx_trace_occlusion is declared, exported and bound, and adds no buffer id."""
import os

import host_support as HS

ROOT = HS.ROOT


def test_the_entry_point_is_declared_exported_and_bound(built):
    HS.declared_exported_bound(
        "rtggx_trace_occlusion",
        r"\bint\s+rtggx_trace_occlusion\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*rays\s*,\s*uint32_t\s+n\s*,\s*uint32_t\s*\*\s*occluded\s*\)",
        defines=(r"\bRTGGX_BUF_COUNT\s*=\s*28\b",))      # nothing new is read back by id


def test_the_header_states_what_an_occluded_ray_does_not_say(built):
    header = open(os.path.join(ROOT, "include", "rtggx.h")).read()
    doc = header[header.index("Occlusion queries"):header.index("rtggx_trace_occlusion(")]
    for word in ("unspecified", "exclusive", "still-sky"):
        assert word in doc, word


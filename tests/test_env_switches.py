"""The environment switches of the library: one struct in csrc/fastsvc_plan.cpp reads them, INTEGRATION.md section 4
lists them (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan_source():
    with open(os.path.join(ROOT, "svcc23_fastsvc_amd", "csrc", "fastsvc_plan.cpp")) as f:
        return f.read()


def _struct_switches(src):
    body = src[src.index("struct Switches {"):src.index("const Switches& env()")]
    return re.findall(r'(?:num|real|given)\("(FASTSVC_[A-Z0-9_]+)"', body)


def test_integration_md_lists_every_switch_of_the_struct():
    names = _struct_switches(_plan_source())
    assert names and len(names) == len(set(names)), names
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    section = doc[doc.index("Run-time switches (environment"):doc.index("## 4b.")]
    listed = set(re.findall(r"FASTSVC_[A-Z0-9_]+", section))
    assert not [n for n in names if n not in listed]
    # ... and the section names nothing the library does not read (FASTSVC_HIP_LIB is the Python loader's; the two
    # FASTSVC_TIMELINE_* of the diagnostic build are read per call; FASTSVC_COND_TRACE doubles as the build's -D flag)
    assert listed - set(names) == {"FASTSVC_HIP_LIB", "FASTSVC_TIMELINE_LAYER", "FASTSVC_TIMELINE_OUT"}


def test_the_environment_is_read_in_the_struct_and_nowhere_else():
    src = _plan_source()
    start, end = src.index("struct Switches {"), src.index("const Switches& env()")
    tl_start = src.index("bool timeline_launch(")
    tl_end = src.index("#endif", tl_start)
    outside = [m.start() for m in re.finditer(r"getenv", src)
               if not (start <= m.start() < end or tl_start <= m.start() < tl_end)]
    assert not outside, [src[max(0, i - 60):i + 40] for i in outside]

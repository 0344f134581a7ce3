"""Golden fixture of what FusedStage2Step launches around its sample set (tests/test_fused_samples_call_sequences_cpu.py, whose
scenario function this runs).

    python tests/golden/make_fused_samples_call_trace.py [checkout]     # writes tests/golden/fused_samples_call_trace.json

`checkout` (default: this tree) is a checkout of the commit that is to be the yardstick, with nothing of the step edited and the
library built: the PACKAGE is imported from there and the file records that checkout's hash (HEAD), while the scenario is this
tree's -- so a commit from before the test existed can be recorded.  The test then holds every later state of fused_step.py and
fused_samples.py to the same calls.  Needs no GPU; the library has to be built, because the argument kinds (pointer or scalar)
are read from the binding derived of its header."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CHECKOUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path.insert(0, ROOT)
if CHECKOUT != ROOT:
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "relightable3dgaussian_amd", os.path.join(CHECKOUT, "relightable3dgaussian_amd", "__init__.py"),
        submodule_search_locations=[os.path.join(CHECKOUT, "relightable3dgaussian_amd")])
    sys.modules["relightable3dgaussian_amd"] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sys.modules["relightable3dgaussian_amd"])
from tests import test_fused_samples_call_sequences_cpu as t  # noqa: E402


def main():
    parent = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=CHECKOUT, text=True).strip()
    with pytest.MonkeyPatch.context() as mp:
        traces = t.scenario(mp)
    doc = t.pack(traces, parent)
    assert t.unpack(json.loads(json.dumps(doc))) == json.loads(json.dumps(traces))
    with open(t.GOLDEN, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s: %d bytes, %d distinct calls, %s" % (t.GOLDEN, os.path.getsize(t.GOLDEN), len(doc["calls"]),
                                                          {k: len(v) for k, v in doc["traces"].items()}))


if __name__ == "__main__":
    main()

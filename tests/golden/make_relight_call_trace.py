"""Golden fixture of what RelightRenderer launches (tests/test_relight_call_sequences_cpu.py, whose scenario function this runs).

    python tests/golden/make_relight_call_trace.py     # writes tests/golden/relight_call_trace.json

Run it on a checkout of the commit that is to be the yardstick, with nothing of the renderer edited: the file records that
commit's hash (HEAD), and the test then holds every later state of relight.py to the same calls.  Needs no GPU; the library has
to be built, because the argument kinds (pointer or scalar) are read from the binding derived of its header."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import test_relight_call_sequences_cpu as t  # noqa: E402


def main():
    parent = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
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

#!/usr/bin/env python3
"""profiles/far_offsets_time.json from the output of the far-offset GPU tests:

    python -m pytest -q -s -m gpu --durations=0 tests/test_gpu_far_offsets_*.py > far.log
    python scripts/far_offsets_time.py far.log > profiles/far_offsets_time.json

Every ``with far_offsets.measured(...)`` block of the tests prints one ``far_offsets_time {json}`` line (the GPU calls and their
comparison: wall seconds with the device synchronised at both ends, the shape, the peak bytes of torch's allocator); pytest's
``--durations`` lines give the wall time of each whole test, the oracle and the building of the inputs included."""
import json
import re
import sys


def main(path):
    blocks, tests = [], {}
    for line in open(path):
        m = re.search(r"far_offsets_time (\{.*\})", line)
        if m:
            blocks.append(json.loads(m.group(1)))
        m = re.match(r"\s*([0-9.]+)s call\s+(tests/test_gpu_far_offsets\S+)", line)
        if m:
            tests[m.group(2)] = float(m.group(1))
    out = {"unit": "seconds of wall time; bytes", "blocks": blocks, "test_calls": dict(sorted(tests.items())),
           "slowest_block": max(blocks, key=lambda b: b["seconds"]) if blocks else None,
           "largest_peak_bytes": max((b["peak_bytes"] for b in blocks), default=0),
           "sum_of_test_calls": round(sum(tests.values()), 2)}
    json.dump(out, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])

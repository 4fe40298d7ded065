"""What every route of a solve enqueues, recorded from the device (tests/golden/solve_sequence_pins.json).

The host side of a solve (solve_begin / solve_end and the launch functions of tdunes_device.hip) decides which launches go out, how many
iterations are enqueued ahead of a read-back, how line-search trials are batched and predicted.  None of that shows in a solution; it
shows in n_launches, in the counts, and in the plan flags.  This script records them for the cases of tests/solve_sequence_cases.py --
three consecutive solves, cold / warm / warm, on fresh mirrors, the sharded modes among them -- on the build it is run on.  test_gpu_solve_sequence.py replays the
cases and asserts equality field for field, so the fixture is recorded BEFORE a change of the host side that is to preserve behaviour,
and re-recorded only by a change that means to alter what is enqueued.

Stability: every case runs three times in fresh mirrors.  A case whose three records differ is written under "unstable" with the
differing fields, and the test skips it; more than two such cases and nothing is written.

Run on the GPU machine: python tools/make_solve_pins.py [--out FILE]
"""
from __future__ import annotations

import json
import sys
import traceback
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))
from treeqp_amd import capi          # noqa: E402
import solve_sequence_cases as SC    # noqa: E402

OUT = ROOT / "tests" / "golden" / "solve_sequence_pins.json"
REPEATS = 3
MAX_UNSTABLE = 2


def differing_fields(runs):
    out = set()
    for other in runs[1:]:
        for s0, s1 in zip(runs[0], other):
            for m0, m1 in zip(s0, s1):
                out |= {k for k in m0 if m0[k] != m1.get(k)}
    return sorted(out)


def main():
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else OUT
    if capi.device_count() < 1:
        raise SystemExit("no HIP device visible")
    pins, unstable, failed = {}, {}, {}
    for c in SC.CASES:
        try:
            runs = [SC.run_case(capi, c) for _ in range(REPEATS)]
            SC.check_case(c, runs[0])
        except Exception:
            failed[c["id"]] = traceback.format_exc()
            print(f"{c['id']}: FAILED\n{failed[c['id']]}", flush=True)
            continue
        diff = differing_fields(runs)
        if diff:
            unstable[c["id"]] = dict(fields=diff, runs=runs)
        else:
            pins[c["id"]] = runs[0]
        for i, solve in enumerate(runs[0]):
            print(f"{c['id']} solve {i}: " + " | ".join(" ".join(f"{k}={v}" for k, v in m.items() if not k.startswith("stage_steps")) for m in solve)
                  + (f"   UNSTABLE {diff}" if diff else ""), flush=True)
    print(f"{len(pins)} cases pinned, {len(unstable)} unstable {sorted(unstable)}, {len(failed)} failed {sorted(failed)}")
    if failed or len(unstable) > MAX_UNSTABLE:
        raise SystemExit("nothing written: a pin that hides these cases would be worth nothing")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(solves=SC.SOLVES, cases=pins, unstable=unstable), indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

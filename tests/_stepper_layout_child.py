"""Child of tests/test_hip_stepper_layouts.py: every 2-D case of tests/stepper_layout_cases.py under this process's SMK_JACOBI_PERSIST (read
once per process), both velocity scales and both fills; one RESULT line of JSON.  Not a test module."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import stepper_layout_cases as S                                      # noqa: E402


def main():
    out = {"cases": {}, "class": {}}
    for H, W, J in S.SHAPES_2D:
        for vel in S.VELS:
            out["class"][f"{H}x{W}-J{J}-{vel}"] = S.run_wrapper_class_2d(H, W, J, vel)
        for layout in S.LAYOUTS:
            runs = {}
            for vel in S.VELS:
                for fill in S.FILLS:
                    r = S.run_case_2d(H, W, J, layout, vel, fill)
                    runs[f"{vel}/{fill}"] = r
                    for what in r["bad"]:
                        print(f"MISMATCH {H}x{W}-J{J}-{layout.name} vel {vel} fill {fill}: {what}", flush=True)
            out["cases"][f"{H}x{W}-J{J}-{layout.name}"] = runs
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

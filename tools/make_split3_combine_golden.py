"""Records tests/golden/split3_combine_parent.json: sha256 of the logits of the teacher-forced windows of tests/split3_cases.py, computed by
a library WITHOUT the slab-wave combine prologue (the commit before it), on a GPU:

    PTTS_LIB=<parent checkout>/parler_tts_amd/libptts_hip.so python tools/make_split3_combine_golden.py <output.json>

tests/test_split3_combine_gpu.py requires the same bytes of the library in the tree."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import split3_cases as SC  # noqa: E402


def main(out):
    assert os.environ.get("PTTS_LIB"), "PTTS_LIB must name the parent commit's library"
    os.environ.pop("PTTS_NO_FUSE_QA", None)
    eng = SC.engine(SC.weights())
    gold = {}
    for name, (P, steps, splits) in sorted(SC.WINDOWS.items()):
        gold[name] = {"prompt": P, "splits": splits, "sha256": [SC.digest(x) for x in SC.step_logits(eng, P, steps)]}
    eng.close()
    with open(out, "w") as f:
        json.dump(gold, f, indent=1)
        f.write("\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main(sys.argv[1])

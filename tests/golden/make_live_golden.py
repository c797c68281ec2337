"""Record tests/golden/live_golden.npz: SHA-256 digests of the GENUINE reference's outputs in the
live cross-checks (tests/test_oracle_golden.py ``test_live_*``, tests/test_unpack_oracle.py
``test_unpack_*_live``), call by call, so that those tests also run where oracle/_ref cannot be
built (tests/canon.py ``Genuine``).

Run where the reference sources are present and `make -C oracle ref` has built oracle/_ref:
    python tests/golden/make_live_golden.py
Every test is recorded in a fresh process: the genuine dense decoder keeps process-wide state.
"""
import inspect
import io
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

OUT = Path(__file__).resolve().parent / "live_golden.npz"
RECORDED = {
    "ascend": ("tests.test_oracle_golden", "test_live_ascend_vs_real_sdk", {}),
    "publish_scan": ("tests.test_oracle_golden", "test_live_publish_scan_vs_real_node", {}),
    "publish_scan_fuzz": ("tests.test_oracle_golden", "test_live_publish_scan_fuzz_vs_real_node", {}),
    **{f"unpack_{ans:#04x}": ("tests.test_unpack_oracle", "test_unpack_matches_genuine_live", {"ans": ans})
       for ans in (0x81, 0x82, 0x83, 0x84, 0x85, 0x86)},
    "unpack_fuzz": ("tests.test_unpack_oracle", "test_unpack_fuzz_vs_genuine_live", {}),
}


def record_one(key):
    """Run one test against the live reference libraries; its digests go to stdout (.npy)."""
    import importlib

    from tests import canon, oracle_lib
    mod, name, kw = RECORDED[key]
    made = []
    genuine = canon.Genuine

    def live_only(k, live):
        if live is None:
            raise SystemExit("oracle/_ref not built: run `make -C oracle ref` where the reference exists")
        made.append(genuine(k, live))
        return made[-1]
    canon.Genuine = live_only
    fn = getattr(importlib.import_module(mod), name)
    args = dict(kw, oracle=oracle_lib.load_oracle())
    if "reflibs" in inspect.signature(fn).parameters:
        args["reflibs"] = oracle_lib.load_ref()
    fn(**args)
    assert [g.key for g in made] == [key], [g.key for g in made]
    buf = io.BytesIO()
    np.save(buf, np.stack(made[0].seen))
    sys.stdout.buffer.write(buf.getvalue())


def main():
    rec = {}
    for key in RECORDED:
        r = subprocess.run([sys.executable, __file__, key], cwd=ROOT, capture_output=True)
        if r.returncode != 0:
            raise SystemExit(f"{key}: {r.stderr.decode()[-2000:]}")
        rec[key] = np.load(io.BytesIO(r.stdout))
        print(key, rec[key].shape[0], "calls")
    np.savez_compressed(OUT, **rec)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        record_one(sys.argv[1])
    else:
        main()

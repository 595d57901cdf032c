"""Record tests/golden/wgrad_parent_bits.json: per shape of tests/wgrad_bits_util.SHAPES the
SHA-256 of the flat gradient, the norm partials and the metrics row after one
hwy_ppo_forward_backward on seeded CPU-drawn inputs.  Run it on an MI355X from the repository
root on the build whose bits are the reference (before a change to ppo_wgrad that must keep
them): python3 tools/record_wgrad_bits.py [output.json].  HWY_LIB overrides the library."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "highway-rope-ppo_amd"), ROOT):
    sys.path.insert(0, p)
import hwy.native as native  # noqa: E402

if os.environ.get("HWY_LIB"):
    native.LIB_PATH = os.environ["HWY_LIB"]
import wgrad_bits_util as wb  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else wb.GOLDEN
rec = {wb.shape_id(c): wb.run_case(c) for c in wb.SHAPES}
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"wrote {len(rec)} shapes to {out}")

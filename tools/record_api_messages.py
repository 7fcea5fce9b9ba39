"""Record the status and rtg_last_error() text of every case of tests/api_message_cases.py against the library
RTG_LIB names (default: the in-tree build) into tests/golden/api_messages.json, {section: {case: [rc, message]}}.

  python tools/record_api_messages.py host     # needs no device; run where none is visible, so the constructors'
                                               # first device call fails and its label is recorded
  python tools/record_api_messages.py gpu      # needs one: live handles, nothing launched beyond their creation

A section is replaced as a whole; the other one is kept.  Record from the build whose messages are the contract
(before a change to csrc/rtg_api.cpp, not after)."""
from __future__ import annotations

import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "humanoid-real-time-retarget_amd"), os.path.join(REPO, "tests")]
OUT = os.path.join(REPO, "tests", "golden", "api_messages.json")


def main():
    import api_message_cases as cases
    from rtg import _lib
    section = sys.argv[1] if len(sys.argv) > 1 else ""
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    if section not in ("host", "gpu"):
        sys.exit(__doc__)
    if section == "gpu":   # torch opens the device first, as in every caller of the package
        import torch
        if not torch.cuda.is_available():
            sys.exit("the gpu section needs a HIP device")
    lib = _lib.lib()
    if section == "host":
        if lib.rtg_device_count() != 0:
            sys.exit("record the host section where no device is visible (the nodev: cases need their failure)")
        res = cases.run(cases.host_cases(lib), lib, True)
    else:
        res = cases.run(cases.gpu_cases(lib), lib, False)
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc[section] = res
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{section}: {len(res)} cases from {_lib.LIB_PATH} -> {out}")


if __name__ == "__main__":
    main()

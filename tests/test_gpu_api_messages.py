"""The C ABI's statuses and messages behind live handles, against the record (tests/golden/api_messages.json, section
"gpu", written on an MI355X by tools/record_api_messages.py).  One process, a dozen tiny handles; every case is an
argument error returned before any launch."""
import json
import os

import pytest

import api_message_cases as cases
from conftest import GOLDEN


@pytest.mark.gpu
def test_gpu_messages_match_the_record(gpu):
    """Every gpu case returns the recorded status and leaves the recorded text in rtg_last_error(), byte for byte:
    the checks behind a live topology (3, 21, 59 and 65 joints), a model without limits, a plan, a rotation-ingest
    handle, a motion library and one solver of each kind.

    The fail( sites of csrc/rtg_api.cpp that neither this section nor the "host" one reaches (the same list as in
    tests/test_api_messages_host.py::test_host_messages_match_the_record), and why:
      - "host allocation failed" of the six constructors: a failed `new` of a small struct cannot be arranged;
      - hip_check behind every device call but a constructor's first: it needs a device that fails part-way, and
        here every handle is created successfully (the first labels are the host section's ``nodev:`` cases);
      - rtg_frame_server_post's "not served within": it needs a running server that stalls; no case launches;
      - take_device_error's "a previous launch reported device error": it needs a launch that sets the word
        (tests/test_gpu_edge.py::test_handover_timeout_is_reported_not_silent does that with a measurement build);
      - rtg_server_inbox_alloc's "not a large-BAR device": an MI355X has a large BAR.
    Nothing else is left out."""
    from rtg import _lib
    lib = _lib.lib()
    with open(os.path.join(GOLDEN, "api_messages.json")) as f:
        want = json.load(f)["gpu"]
    got = cases.run(cases.gpu_cases(lib), lib, False)
    assert sorted(got) == sorted(want), set(got) ^ set(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong

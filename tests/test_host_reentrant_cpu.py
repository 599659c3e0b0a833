"""The host mirror (radio-observer_amd/host) formats times on two threads at once: SnapshotRecorder's worker writes a
file (DATE, DATE-OBS) while the stream's thread names the next snapshot.  Neither may go through the C library's one
shared struct tm (gmtime, localtime, ctime, asctime): the name of a snapshot once came out with the hour, minute and
second of the DATE card being written beside it."""
import os
import re

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radio-observer_amd", "host")


def test_host_time_formatting_is_reentrant():
    sources = sorted(f for f in os.listdir(HOST) if f.endswith((".cpp", ".h")))
    assert len(sources) >= 10
    for name in sources:
        code = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(HOST, name)).read(), flags=re.S)
        assert not re.search(r"\b(?:gmtime|localtime|ctime|asctime)\s*\(", code), name

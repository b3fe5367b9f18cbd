"""The SN_* environment switches of the library live in ONE table, hobot_stereonet_amd/csrc/sn_switches.hpp (struct Switches:
one field per switch with its variable, default, scope and meaning), and INTEGRATION.md §3 documents the same list.  Text
checks only: no build, no device."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hobot_stereonet_amd", "csrc")
TABLE = os.path.join(CSRC, "sn_switches.hpp")
# a field's comment: // SN_NAME | default | process or create | meaning
ROW = re.compile(r"//\s*(SN_[A-Z0-9_]+)\s*\|\s*([^|]+?)\s*\|\s*(process|create)\s*\|\s*(\S.*)")


def _table():
    rows = {}
    for line in open(TABLE).read().splitlines():
        m = ROW.search(line)
        if m:
            assert m.group(1) not in rows, f"{m.group(1)} is in the table twice"
            rows[m.group(1)] = (m.group(2), m.group(3), m.group(4))
    return rows


def _integration_section3():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = text.index("\n## 3. ")
    return text[start:text.index("\n## 4. ", start)]


def _abi_names():
    return set(re.findall(r"\bSN_[A-Z0-9_]+", open(os.path.join(ROOT, "include", "stereonet_hip.h")).read()))


def test_the_table_has_every_switch_with_default_scope_and_meaning():
    rows = _table()
    assert len(rows) >= 27, sorted(rows)
    for name in ("SN_DOWN01", "SN_FUSE", "SN_STREAM_WGS", "SN_FIRST_PIECE", "SN_ASYNC_SHARE"):
        assert rows[name][1] == "process", (name, rows[name])
    for name in ("SN_W_ROUND", "SN_PRECISION", "SN_TOWER_STREAMS", "SN_STREAM_PRIORITY", "SN_NO_OVERLAP", "SN_NO_GRAPH",
                 "SN_TAIL_FUSE", "SN_MGPU_GATHER", "SN_MGPU_ALLOW_DUP"):
        assert rows[name][1] == "create", (name, rows[name])
    # every variable the fill function reads has a row, and every row is read
    read = set(re.findall(r'"(SN_[A-Z0-9_]+)"', open(TABLE).read()))
    assert read == set(rows), (sorted(read - set(rows)), sorted(set(rows) - read))


def test_no_getenv_of_a_switch_outside_the_table():
    offenders = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(CSRC, "*.h"))):
        if os.path.samefile(path, TABLE):
            continue
        for no, line in enumerate(open(path).read().splitlines(), 1):
            if re.search(r'getenv\s*\(\s*"SN_', line):
                offenders.append(f"{os.path.basename(path)}:{no}: {line.strip()}")
    assert not offenders, offenders


def test_every_switch_of_the_table_is_documented():
    doc = _integration_section3()
    missing = [name for name in _table() if not re.search(r"\b" + name + r"\b", doc)]
    assert not missing, missing


def test_every_documented_switch_is_in_the_table():
    rows, abi = _table(), _abi_names()
    unknown = []
    for name in sorted(set(re.findall(r"\bSN_[A-Z0-9_]*[A-Z0-9]", _integration_section3()))):
        if name in ("SN_LOG_LEVEL", "SN_ROOT") or name in rows:
            continue
        if any(a == name or a.startswith(name + "_") for a in abi):      # ABI enums and macros (SN_PREC_AUTO, SN_LRC_*, ...)
            continue
        unknown.append(name)
    assert not unknown, unknown

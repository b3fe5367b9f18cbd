"""The `key value...` text files of the tools and the node's stages: one reader and one writer under every module's
``load_params`` / ``save_params`` (and ``rectify.load_calib`` / ``save_calib``).  One key a line, ``#`` starts a comment, a key
at most once.  The node's reader is csrc/compat/src/param_file.cpp; DESIGN.md says where the two differ.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, NamedTuple, Tuple


class Key(NamedTuple):
    """what a key's line holds: `count` values, each through `conv` (float, int or str); repeat: the key may come again, and
    its lines are collected in a list"""
    count: int = 1
    conv: Callable = float
    repeat: bool = False


def spec(floats: Iterable[str] = (), ints: Iterable[str] = (), **others: Key) -> Dict[str, Key]:
    return {**{k: Key(1, float) for k in floats}, **{k: Key(1, int) for k in ints}, **others}


def read(path: str, keys: Dict[str, Key], required: bool = False) -> dict:
    """key -> its value (a tuple where count > 1, a list of them for a repeat key), for the keys the file has.  ValueError with
    `path:line:` in front for an unknown or repeated key, a wrong number of values or a value conv refuses; with required, for
    a key of `keys` that the file lacks."""
    got: dict = {}
    with open(path) as f:
        for no, text in enumerate(f, 1):
            words = text.split("#", 1)[0].split()
            if not words:
                continue
            name, vals = words[0], words[1:]
            if name not in keys:
                raise ValueError(f"{path}:{no}: unknown key {name!r}")
            key = keys[name]
            if (name in got and not key.repeat) or len(vals) != key.count:
                raise ValueError(f"{path}:{no}: expected one `{name}` line with {key.count} value{'s' if key.count > 1 else ''}")
            try:
                nums = tuple(key.conv(v) for v in vals)
            except ValueError:
                raise ValueError(f"{path}:{no}: not a number in {text.strip()!r}") from None
            value = nums if key.count > 1 else nums[0]
            if key.repeat:
                got.setdefault(name, []).append(value)
            else:
                got[name] = value
    missing = [k for k in keys if k not in got] if required else []
    if missing:
        raise ValueError(f"{path}: missing {', '.join(missing)}")
    return got


def write(path: str, header: str, keys: Dict[str, Key], lines: Iterable[Tuple[str, object]]) -> None:
    """`# header`, then one `key value...` line per (key, value or values): floats as repr, so that read gives them back exactly"""
    def word(conv, v) -> str:
        return v if conv is str else repr(float(v)) if conv is float else str(int(v))
    with open(path, "w") as f:
        f.write("# " + header + "\n")
        for name, value in lines:
            key = keys[name]
            f.write(name + " " + " ".join(word(key.conv, v) for v in (value if key.count > 1 else (value,))) + "\n")

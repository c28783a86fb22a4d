"""The one reader of the C header (include/terrarium_hip.h) for the tests: its enumerators, integer #defines and declared entry points,
and the Python-side table the naming rule gives for an enum prefix -- strip the prefix, lower-case the rest."""
import os
import re

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "terrarium_hip.h")
_INTEGER = r"[ \t0-9a-fA-FxXuUlL()<+-]+"         # decimal, hex, `u` suffixes, shifts, sums, parentheses: 4u, 0x1F, 1u << 3, (-2147483647 - 1)


def text() -> str:
    with open(PATH) as f:
        return f.read()


def _code(source):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text() if source is None else source, flags=re.S)


def _value(expr: str) -> int:
    assert re.fullmatch(_INTEGER, expr), expr
    return int(eval(re.sub(r"(?<=[0-9a-fA-F])[uUlL]+\b", "", expr), {}))


def enums(source=None) -> dict:
    """{name: value} of every enumerator; one without a value of its own counts on from the one before it"""
    out = {}
    for body in re.findall(r"\benum\s*\w*\s*\{([^}]*)\}", _code(source)):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, expr = (" ".join(part.split()) for part in item.partition("="))
            value = _value(expr) if expr else value + 1
            assert name not in out, name
            out[name] = value
    return out


def defines(source=None) -> dict:
    """{name: value} of the #defines with an integer value"""
    return {name: _value(expr) for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(%s?)[ \t]*$" % _INTEGER, _code(source), flags=re.M)}


def functions(source=None) -> list:
    """the declared trm_* entry points, sorted"""
    return sorted(set(re.findall(r"\b(trm_[a-z_0-9]+)\s*\(", _code(source))))


def table(prefix: str, aliases=None, exclude=(), source=None) -> dict:
    """The enumerators `prefix`*, but those whose rest starts with one of `exclude`, by their Python names: the rest in lower case,
    or what `aliases` gives for it"""
    rest = {name[len(prefix):]: value for name, value in enums(source).items() if name.startswith(prefix)}
    return {(aliases or {}).get(r, r.lower()): v for r, v in rest.items() if not r.startswith(tuple(exclude))}

"""What the ABI tests read of include/*.h: a header without its comments, the symbols it declares, and the names the
binding table (eogs2_amd._abi.HEADERS) holds under the other headers."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def header_text(name):
    """include/<name> with its comments stripped (the headers are C: /* */ only)."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def declared(name):
    """{symbol: number of parameters} of every eogs_* function include/<name> declares."""
    out = {}
    for sym, params in re.findall(r"\b(eogs_[a-z_0-9]+)\s*\(([^)]*)\)", header_text(name)):
        n = len([p for p in params.split(",") if p.strip() and p.strip() != "void"])
        assert out.setdefault(sym, n) == n, f"{name}: {sym} is declared twice, differently"
    return out


def elsewhere(name):
    """Every name the binding table holds under a header other than `name`."""
    from eogs2_amd._abi import HEADERS

    return {sym for h, table in HEADERS.items() if h != name for sym in table}

"""The model of the validator-set history (include/edc.h, edc_vhist_*), and the generator of
tests/golden/vhist.json.     Run: python tests/golden/gen_vhist.py   (seconds, no oracle)

The entries are the validator-set entries (gen_valset.py) with the set kept as a base plus
per-version updates: every commit names the version it is judged by, and a vote's signer is a
member, with a power, only as that version says. The model below restates the header's definitions
in plain Python on top of gen_valset's and gen_quorum's: the rules of edc_vhist_set, the state of
every version, the change lists, the totals, the join and everything behind it. It is imported by
tests/test_vhist_abi.py and tests/test_gpu_vhist.py.

vhist.json holds a few small histories laid out by hand for the situations the header names
(HISTORIES below) with what the model says about each. DATA only.
"""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _gen_valset():
    spec = importlib.util.spec_from_file_location("gen_valset", os.path.join(HERE, "gen_valset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


V = _gen_valset()
Q = V.Q
OK, INVALID, SHORT, DOUBLE_VOTE, NOT_CHECKED = V.OK, V.INVALID, V.SHORT, V.DOUBLE_VOTE, V.NOT_CHECKED
ABSENT, COMMIT, NIL = V.ABSENT, V.COMMIT, V.NIL
FULL, LIGHT = V.FULL, V.LIGHT
MAX_POWER, NO_POS = V.MAX_POWER, V.NO_POS
NOT_MEMBER = 0xFFFFFFFFFFFFFFFF          # EDC_VHIST_NOT_MEMBER

# why edc_vhist_set refuses a history, in the order the checks are made
REFUSALS = ("list", "length", "offsets", "count", "keys", "position", "power", "sum", "twice")


# ---------------------------------------------------------------- the model
def build(keys, m, base, upd_off, upd_pos, upd_power):
    """edc_vhist_set on the registered list `keys` (None or []: there is none): m base powers and the
    updates as the C arrays (upd_off has nv + 1 entries). Returns one of REFUSALS, or the history:
    a dict with m, nv, states (the power of every position at every version, NOT_MEMBER included),
    the change lists off / ver / pow by position, total and members."""
    if not keys:
        return "list"
    if m != len(keys) or len(base) != m:
        return "length"
    nv = len(upd_off) - 1 if upd_off else 0
    if nv and (upd_off[0] != 0 or any(b < a for a, b in zip(upd_off, upd_off[1:]))):
        return "offsets"
    nu = upd_off[nv] if nv else 0
    if m + nu >= 1 << 32:
        return "count"
    if len(set(bytes(k) for k in keys)) != len(keys):
        return "keys"
    if any(p >= m for p in upd_pos[:nu]):
        return "position"
    if any(w != NOT_MEMBER and w > MAX_POWER for w in base):
        return "power"
    lists = [[(0, w)] for w in base]
    states = [list(base)]
    for v in range(nv + 1):
        if sum(w for w in states[v] if w != NOT_MEMBER) > MAX_POWER:
            return "sum"
        if v == nv:
            break
        cur, seen = list(states[v]), set()
        for j in range(upd_off[v], upd_off[v + 1]):
            p, w = upd_pos[j], upd_power[j]
            if p in seen:
                return "twice"
            seen.add(p)
            if w != NOT_MEMBER and w > MAX_POWER:
                return "power"
            cur[p] = w
            lists[p].append((v + 1, w))
        states.append(cur)
    off = [0]
    for l in lists:
        off.append(off[-1] + len(l))
    return {"m": m, "nv": nv, "states": states, "off": off,
            "ver": [v for l in lists for v, _ in l], "pow": [w for l in lists for _, w in l],
            "total": [sum(w for w in s if w != NOT_MEMBER) for s in states],
            "members": [sum(1 for w in s if w != NOT_MEMBER) for s in states]}


def from_updates(keys, base, updates):
    """build() from one list of (position, power) pairs per version 1..nv, as Engine.vhist_set takes them"""
    off = [0]
    for u in updates:
        off.append(off[-1] + len(u))
    flat = [x for u in updates for x in u]
    return build(keys, len(base), list(base), off if updates else [], [p for p, _ in flat], [w for _, w in flat])


def power_at(h, p, v):
    """the power of position p at version v (NOT_MEMBER: no member then), straight from the definition"""
    return h["states"][v][p]


def lookup(h, p, v):
    """the same from the change list: the last entry of position p with ver <= v"""
    best = None
    for j in range(h["off"][p], h["off"][p + 1]):
        if h["ver"][j] <= v:
            best = h["pow"][j]
    return best


def resolve(keys, h, off, versions, flag, vks=None, key_idx=None):
    """The join -> (pos, power, flag_out). Exactly one of vks (key bytes) and key_idx (positions in keys).
    A flag above 2 is passed through whoever signed."""
    assert (vks is None) != (key_idx is None) and len(versions) == len(off) - 1
    assert all(0 <= v <= h["nv"] for v in versions)
    where = {bytes(k): p for p, k in enumerate(keys)}
    pos, power, flag_out = [], [], []
    for c, (a, e) in enumerate(zip(off, off[1:])):
        for i in range(a, e):
            p = where.get(bytes(vks[i]), NO_POS) if key_idx is None else key_idx[i]
            w = NOT_MEMBER if p == NO_POS else power_at(h, p, versions[c])
            member = w != NOT_MEMBER
            pos.append(p if member else NO_POS)
            power.append(w if member else 0)
            flag_out.append(flag[i] if member or flag[i] > NIL else ABSENT)
    return pos, power, flag_out


def plan(keys, h, off, versions, flag, thr, mode, vks=None, key_idx=None):
    """Everything edc_vhist_resolve returns, as Engine.vhist_resolve's dict."""
    pos, power, flag_out = resolve(keys, h, off, versions, flag, vks, key_idx)
    checked, planned = Q.select(off, power, flag_out, thr, mode)
    return {"pos": pos, "power": power, "flag": flag_out, "checked": checked, "planned": planned,
            "n_checked": sum(checked), "dv": V.double_votes(off, pos, checked)}


def judge(keys, h, off, versions, flag, thr, mode, codes, vks=None, key_idx=None):
    """Everything a verify call returns but check8, from the items' verify_single codes: the quorum
    entries' results on the joined power / flag, then the double-vote verdicts and the return value."""
    p = plan(keys, h, off, versions, flag, thr, mode, vks, key_idx)
    j = Q.judge(off, p["power"], p["flag"], thr, mode, codes)
    assert j["checked"] == p["checked"] and j["planned"] == p["planned"]
    j["quorum_verdicts"], j["quorum_code"] = list(j["commit_verdicts"]), j["code"]
    j["commit_verdicts"] = [DOUBLE_VOTE if d else v for d, v in zip(p["dv"], j["commit_verdicts"])]
    v = j["commit_verdicts"]
    j["code"] = INVALID if INVALID in v else DOUBLE_VOTE if DOUBLE_VOTE in v else SHORT if SHORT in v else OK
    j["n_bad_commits"] = sum(1 for x in v if x != OK)
    j.update(pos=p["pos"], power=p["power"], flag=p["flag"], dv=p["dv"])
    return j


# ---------------------------------------------------------------- the recorded histories
def _key(i):
    return bytes([i + 1]) * 32


KEYS = [_key(i) for i in range(4)]
N = NOT_MEMBER
# four positions; what the header's rules say about each is asserted by hand in tests/test_vhist_abi.py
HISTORIES = {
    # position 2 is absent at the base, joins at version 2, leaves at 4 and rejoins at 5
    "join_leave_rejoin": {"base": [5, 5, N, 7], "updates": [[], [(2, 9)], [(0, 6)], [(2, N)], [(2, 4)], []]},
    # one update at exactly version 3, looked at from versions 2, 3 and 4
    "update_at_v": {"base": [1, 2, 3, 4], "updates": [[], [], [(1, 20)], []]},
    # a member with power 0 is a member: it counts in members, not in total; then it leaves
    "zero_power": {"base": [0, 3, N, N], "updates": [[(1, 0)], [(0, N)]]},
    # an update that restates the state changes no version
    "restated": {"base": [5, N, 5, 5], "updates": [[(0, 5), (1, N)], [(2, 6)]]},
}


def recorded(name):
    c = HISTORIES[name]
    h = from_updates(KEYS, c["base"], c["updates"])
    return {k: h[k] for k in ("nv", "states", "off", "ver", "pow", "total", "members")}


def main():
    out = {"not_member": NOT_MEMBER, "histories": {name: recorded(name) for name in HISTORIES}}
    with open(os.path.join(HERE, "vhist.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    for name, h in out["histories"].items():
        print(name, h["total"], h["members"])


if __name__ == "__main__":
    main()

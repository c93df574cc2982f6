"""The model of the validator-set quorum commit sets (include/edc.h, edc_valset_*), and the generator of
tests/golden/valset.json.     Run: python tests/golden/gen_valset.py   (seconds, no oracle)

The entries are the quorum entries (gen_quorum.py) with the powers kept beside the registered key
list: every vote's signer is joined against that list, a signer the list does not know counts as
absent, and a commit in which one member has two CHECKED votes is a double vote. The model below
restates the header's definitions in plain Python on top of gen_quorum's: the rules of
edc_valset_set_powers, the join, the double-vote rule, the verdicts and the return value. It is
imported by tests/test_valset_abi.py and tests/test_gpu_valset.py.

valset.json holds a few small sets laid out by hand for the situations the header names (CASES
below) with what the model says about each in both modes; nothing is signed here, the item codes
are given. DATA only.
"""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _gen_quorum():
    spec = importlib.util.spec_from_file_location("gen_quorum", os.path.join(HERE, "gen_quorum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


Q = _gen_quorum()
OK, INVALID, SHORT, DOUBLE_VOTE, NOT_CHECKED = Q.OK, Q.INVALID, Q.SHORT, 4, Q.NOT_CHECKED
ABSENT, COMMIT, NIL = Q.ABSENT, Q.COMMIT, Q.NIL
FULL, LIGHT = Q.FULL, Q.LIGHT
MAX_POWER = Q.MAX_POWER
NO_POS = 0xFFFFFFFF


# ---------------------------------------------------------------- the model
def check_powers(keys, powers, m=None):
    """edc_valset_set_powers: True iff powers (m of them) are accepted for the registered list keys."""
    m = len(powers) if m is None else m
    if not keys or m != len(keys) or len(set(bytes(k) for k in keys)) != len(keys):
        return False
    return all(0 <= p <= MAX_POWER for p in powers) and sum(powers) <= MAX_POWER


def resolve(keys, powers, flag, vks=None, key_idx=None):
    """The join -> (pos, power, flag_out). Exactly one of vks (key bytes) and key_idx (positions in keys)."""
    assert (vks is None) != (key_idx is None)
    if key_idx is None:
        where = {bytes(k): p for p, k in enumerate(keys)}
        pos = [where.get(bytes(v), NO_POS) for v in vks]
    else:
        pos = list(key_idx)
    power = [0 if p == NO_POS else powers[p] for p in pos]
    flag_out = [ABSENT if p == NO_POS else f for p, f in zip(pos, flag)]
    return pos, power, flag_out


def check_args(off, flag, power, flag_out):
    """What the device refuses: a flag above 2 on any item, a commit whose counted sum passes 2^63 - 1."""
    return all(f in (ABSENT, COMMIT, NIL) for f in flag) and Q.check_args(off, power, flag_out, None)


def double_votes(off, pos, checked):
    """dv[c] = 1 iff two checked items of commit c resolve to the same member."""
    dv = []
    for a, e in zip(off, off[1:]):
        seen = [pos[i] for i in range(a, e) if checked[i] and pos[i] != NO_POS]
        dv.append(int(len(set(seen)) != len(seen)))
    return dv


def plan(keys, powers, off, flag, thr, mode, vks=None, key_idx=None):
    """Everything edc_valset_resolve returns, as Engine.valset_resolve's dict."""
    pos, power, flag_out = resolve(keys, powers, flag, vks, key_idx)
    checked, planned = Q.select(off, power, flag_out, thr, mode)
    return {"pos": pos, "power": power, "flag": flag_out, "checked": checked, "planned": planned,
            "n_checked": sum(checked), "dv": double_votes(off, pos, checked)}


def judge(keys, powers, off, flag, thr, mode, codes, vks=None, key_idx=None):
    """Everything a verify call returns but check8, from the items' verify_single codes: the quorum
    entries' results on the joined power / flag, then the double-vote verdicts and the return value."""
    p = plan(keys, powers, off, flag, thr, mode, vks, key_idx)
    j = Q.judge(off, p["power"], p["flag"], thr, mode, codes)
    assert j["checked"] == p["checked"] and j["planned"] == p["planned"]
    j["quorum_verdicts"], j["quorum_code"] = list(j["commit_verdicts"]), j["code"]
    j["commit_verdicts"] = [DOUBLE_VOTE if d else v for d, v in zip(p["dv"], j["commit_verdicts"])]
    v = j["commit_verdicts"]
    j["code"] = INVALID if INVALID in v else DOUBLE_VOTE if DOUBLE_VOTE in v else SHORT if SHORT in v else OK
    j["n_bad_commits"] = sum(1 for x in v if x != OK)
    j.update(pos=p["pos"], power=p["power"], flag=p["flag"], dv=p["dv"])
    return j


# ---------------------------------------------------------------- the recorded cases
def _key(i):
    return bytes([i + 1]) * 32


# a list of five members with powers 5, 5, 5, 5, 7 (total 27; 2/3 -> 18); "x" is nobody's key.
# Items are (signer, flag); codes default to OK.
KEYS = [_key(i) for i in range(5)]
POWERS = [5, 5, 5, 5, 7]
STRANGER = b"\xee" * 32
CASES = {
    # the second vote of member 1 arrives while the running sum (10) is still <= 10: checked -> dv in light mode
    "second_before_quorum": {"commits": [[(0, 1), (1, 1), (1, 1), (2, 1)]], "thr": [10]},
    # ... and after the sum (10) has passed 9: not checked in light mode, checked in full mode
    "second_after_quorum": {"commits": [[(0, 1), (1, 1), (1, 1), (2, 1)]], "thr": [9]},
    "commit_and_nil": {"commits": [[(0, 1), (3, 2), (3, 1), (4, 1)]], "thr": [30]},
    "three_times": {"commits": [[(2, 1), (2, 1), (0, 1), (2, 1)]], "thr": [30]},
    "two_commits_one_validator": {"commits": [[(0, 1), (1, 1)], [(1, 1), (2, 1)]], "thr": [30, 30]},
    "strangers_twice": {"commits": [[("x", 1), ("x", 1), (0, 1), ("x", 2)]], "thr": [0]},
    "last_commit_then_empty": {"commits": [[(0, 1)], [], [(4, 1), (4, 1)], [], []], "thr": [0, 0, 30, 0, 0]},
    # a double vote beside an invalid commit, and beside a short one: the precedence of the return value
    "with_invalid": {"commits": [[(0, 1), (0, 1)], [(1, 1), (2, 1)], [(3, 1), (4, 1)]], "thr": [30, 1, 1],
                     "codes": {"3": 1}},
    "with_short": {"commits": [[(0, 1), (0, 1)], [(1, 1)], [(3, 1), (4, 1)]], "thr": [30, 30, 1]},
    # the double-vote commit's own second vote is the bad one: still a double vote, its code stays
    "double_and_bad": {"commits": [[(0, 1), (0, 1)], [(1, 1)]], "thr": [30, 1], "codes": {"1": 1}},
}


def case(name):
    c = CASES[name]
    off, vks, flag = [0], [], []
    for items in c["commits"]:
        for who, f in items:
            vks.append(STRANGER if who == "x" else KEYS[who])
            flag.append(f)
        off.append(len(vks))
    codes = [OK] * len(vks)
    for i, v in c.get("codes", {}).items():
        codes[int(i)] = v
    return off, vks, flag, list(c["thr"]), codes


def expected(name):
    off, vks, flag, thr, codes = case(name)
    out = {}
    for mode, label in ((FULL, "full"), (LIGHT, "light")):
        j = judge(KEYS, POWERS, off, flag, thr, mode, codes, vks=vks)
        out[label] = {k: j[k] for k in ("pos", "power", "flag", "checked", "planned", "dv", "item_verdicts", "tally",
                                        "commit_verdicts", "n_checked", "n_bad_commits", "code")}
    return out


def main():
    out = {"powers": POWERS, "cases": {name: expected(name) for name in CASES}}
    with open(os.path.join(HERE, "valset.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    for name, e in out["cases"].items():
        print(name, {m: (e[m]["code"], e[m]["dv"], e[m]["commit_verdicts"]) for m in ("full", "light")})


if __name__ == "__main__":
    main()

"""Generate tests/golden/quorum.json.     Run: python tests/golden/gen_quorum.py   (seconds, no oracle)

Quorum commit sets (include/edc.h, edc_quorum_*): a commit set whose items carry a voting power and
a flag (0 absent, 1 commit, 2 nil) and whose commits carry a threshold. The model below restates
the header's definitions in plain Python: which items are checked in full and in light mode, the
tally a commit gets, its verdict, the set's return code. It is the oracle for everything that is
not a signature, and it is imported by tests/test_quorum_abi.py and tests/test_gpu_quorum.py.

The signed sets are gen_commits.build("valid") and build("mixed_a") with their overrides; the
items' codes are those of commits.json (the CPU oracle judged every item there), so nothing is
signed here. Powers, flags and thresholds are laid down by RULE (votes() below) from the parameters
in RULE, which the file repeats, and the file holds what the model says about the result per mode:
the SHA-256 of the checked bitmap, planned, tally, commit verdicts, n_checked, n_bad_commits, code.
The rule places, in mixed_a (situations(), checked when generating and by the CPU test):
  after    a commit whose bad item comes after its quorum: Ok in light mode, invalid in full mode
  before   a commit whose bad item comes before its quorum: invalid in both
  missing  a commit that is short only because its bad item's power is missing: still invalid
  nil_bad  a nil vote with a bad signature: invalid in full mode, not checked in light mode
  garbage  an absent item whose key and signature bytes are noise, and the ZIP215 corpus commit
DATA only.
"""
import hashlib
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

OK, INVALID, SHORT, NOT_CHECKED = 0, 1, 3, 255
ABSENT, COMMIT, NIL = 0, 1, 2
FULL, LIGHT = 0, 1
MAX_POWER = 2**63 - 1

RULE = {
    "power_mod": 1000,          # power = 1 + (two stream bytes, little endian) % power_mod
    "absent_below": 20,         # third stream byte: < absent_below absent, < nil_below nil, else commit
    "nil_below": 36,
    "sets": {
        "valid": {"flags": {}, "tight_commits": [], "garbage": []},
        "mixed_a": {
            # the five bad items of commits.json: four count as commits, the s = l one is a nil vote
            "flags": {"346": COMMIT, "645": COMMIT, "700": COMMIT, "800": NIL, "2047": COMMIT, "1000": ABSENT},
            "tight_commits": [6],   # threshold = the commit's counted power - 1: every counted vote is needed
            "garbage": [1000],      # absent: vk and sig replaced by stream bytes
        },
    },
}


def _gen_commits():
    spec = importlib.util.spec_from_file_location("gen_commits", os.path.join(HERE, "gen_commits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- the model
def check_args(off, power, flag, thr):
    """The argument rules: True iff a call with these votes is accepted."""
    if any(f not in (ABSENT, COMMIT, NIL) for f in flag) or any(p > MAX_POWER for p in power):
        return False
    return all(sum(p for p, f in zip(power[a:e], flag[a:e]) if f == COMMIT) <= MAX_POWER
               for a, e in zip(off, off[1:]))


def select(off, power, flag, thr, mode):
    """(checked[i], planned[c]): the items that are verified and the tally each commit gets if all of them verify."""
    checked, planned = [0] * (off[-1] if off else 0), []
    for c, (a, e) in enumerate(zip(off, off[1:])):
        run = 0
        for i in range(a, e):
            if mode == LIGHT:
                chk = flag[i] == COMMIT and run <= thr[c]       # the quorum was not yet reached on arrival
            else:
                chk = flag[i] in (COMMIT, NIL)
            if chk and flag[i] == COMMIT:
                run += power[i]
            checked[i] = int(chk)
        planned.append(run)
    return checked, planned


def judge(off, power, flag, thr, mode, codes):
    """Everything a verify call returns but check8, from the items' verify_single codes."""
    checked, planned = select(off, power, flag, thr, mode)
    item = [codes[i] if checked[i] else NOT_CHECKED for i in range(len(checked))]
    tally, verdicts = [], []
    for c, (a, e) in enumerate(zip(off, off[1:])):
        t = sum(power[i] for i in range(a, e) if checked[i] and flag[i] == COMMIT and codes[i] == OK)
        bad = any(checked[i] and codes[i] != OK for i in range(a, e))
        tally.append(t)
        verdicts.append(INVALID if bad else OK if t > thr[c] else SHORT)      # strictly greater
    code = INVALID if INVALID in verdicts else SHORT if SHORT in verdicts else OK
    return {"checked": checked, "planned": planned, "item_verdicts": item, "tally": tally, "commit_verdicts": verdicts,
            "n_bad_commits": sum(1 for v in verdicts if v != OK), "n_checked": sum(checked), "code": code}


# ---------------------------------------------------------------- the rule
def votes(name, off, gc=None):
    """(power, flag, threshold) of a set by RULE; threshold floor(2T/3), T the power of the whole commit."""
    gc = gc or _gen_commits()
    r, n = RULE["sets"][name], off[-1]
    s = gc.stream("quorum/" + name, 3 * n)
    power = [1 + (s[3 * i] | s[3 * i + 1] << 8) % RULE["power_mod"] for i in range(n)]
    flag = [ABSENT if s[3 * i + 2] < RULE["absent_below"] else NIL if s[3 * i + 2] < RULE["nil_below"] else COMMIT
            for i in range(n)]
    for i, f in r["flags"].items():
        flag[int(i)] = f
    thr = [2 * sum(power[a:e]) // 3 for a, e in zip(off, off[1:])]
    for c in r["tight_commits"]:
        thr[c] = sum(p for p, f in zip(power[off[c]:off[c + 1]], flag[off[c]:off[c + 1]]) if f == COMMIT) - 1
    return power, flag, thr


def garbage(name, gc=None):
    """[(item, vk, sig)]: the noise an absent item of the set carries instead of a key and a signature."""
    gc = gc or _gen_commits()
    return [(i, gc.stream("quorum/garbage/vk%d" % i, 32), gc.stream("quorum/garbage/sig%d" % i, 64))
            for i in RULE["sets"][name]["garbage"]]


def item_codes(name):
    with open(os.path.join(HERE, "commits.json")) as f:
        s = json.load(f)["sets"][name]
    codes = [OK] * s["n"]
    for i, c in s["item_codes"].items():
        codes[int(i)] = c
    return codes


def situations(off, power, flag, thr, codes, corpus_commit):
    """Which of the listed mixed_a situations the votes contain: {name: [commits or items]}."""
    full, light = judge(off, power, flag, thr, FULL, codes), judge(off, power, flag, thr, LIGHT, codes)
    allok = judge(off, power, flag, thr, LIGHT, [OK] * len(codes))
    found = {"after": [], "before": [], "missing": [], "nil_bad": [], "garbage": [], "corpus": []}
    for c, (a, e) in enumerate(zip(off, off[1:])):
        bad = [i for i in range(a, e) if codes[i] != OK and flag[i] == COMMIT]
        if bad and light["commit_verdicts"][c] == OK and full["commit_verdicts"][c] == INVALID:
            found["after"].append(c)
        if bad and light["commit_verdicts"][c] == INVALID and full["commit_verdicts"][c] == INVALID:
            found["before"].append(c)
            if allok["commit_verdicts"][c] == OK and light["tally"][c] <= thr[c]:
                found["missing"].append(c)
        for i in range(a, e):
            if codes[i] != OK and flag[i] == NIL and full["item_verdicts"][i] != OK and light["item_verdicts"][i] == NOT_CHECKED \
                    and full["commit_verdicts"][c] == INVALID:
                found["nil_bad"].append(i)
    if corpus_commit is not None and full["commit_verdicts"][corpus_commit] == OK and light["n_checked"]:
        found["corpus"].append(corpus_commit)
    return found


def expected(name, gc=None):
    gc = gc or _gen_commits()
    off = gc.build(name)["commit_off"]
    power, flag, thr = votes(name, off, gc)
    codes = item_codes(name)
    assert check_args(off, power, flag, thr)
    out = {"n": off[-1], "nc": len(off) - 1}
    for mode, label in ((FULL, "full"), (LIGHT, "light")):
        j = judge(off, power, flag, thr, mode, codes)
        out[label] = {"checked_sha256": hashlib.sha256(bytes(j["checked"])).hexdigest(), "planned": j["planned"],
                      "tally": j["tally"], "commit_verdicts": j["commit_verdicts"], "n_checked": j["n_checked"],
                      "n_bad_commits": j["n_bad_commits"], "code": j["code"]}
    return out


def main():
    gc = _gen_commits()
    out = {"rule": RULE, "sets": {name: expected(name, gc) for name in RULE["sets"]}}
    b = gc.build("mixed_a")
    power, flag, thr = votes("mixed_a", b["commit_off"], gc)
    found = situations(b["commit_off"], power, flag, thr, item_codes("mixed_a"), b["corpus_commit"])
    for i, _, _ in garbage("mixed_a", gc):
        assert flag[i] == ABSENT
        found["garbage"].append(i)
    assert all(found.values()), found
    out["sets"]["mixed_a"]["situations"] = found
    with open(os.path.join(HERE, "quorum.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    for name, s in out["sets"].items():
        print(name, {m: (s[m]["code"], s[m]["n_checked"], s[m]["n_bad_commits"]) for m in ("full", "light")})
    print("mixed_a situations:", found)


if __name__ == "__main__":
    main()

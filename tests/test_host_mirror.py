"""What the host knows of each env (csrc/sdc_mirror.hpp), without a GPU: the header compiled by g++ alone into a program that reads
operations and prints the mirror's full state after each, held to
  * a model restated here in Python that shares no text with the header -- eager per-env lists, no pending counter, every derived value
    computed from scratch -- over seeded random sequences of a few thousand operations (short episodes: ends, auto-resets and mark
    overruns are frequent),
  * cases written out by hand from the documented invariants,
  * and the same program built with -fsanitize=address,undefined, run over the same input.

An operation line and what it calls (the driver keeps, per env, the serial of the last mark it asked for; `alive` is about that one):
  I N T F            SdcHostMirror(N, T, F)                 C / L ids[N]        set_cfg_ids / set_loc_ids
  G (x cfg loc)[N]   both, as fields of records             S n                 stepped(n) -> 1: an env just finished
  E                  finished_envs_reset()                  R 0 | R 1 mask[N]   reset(whole batch | mask)
  K n (src dst)[n]   copy_envs                              P n (env t feat cfg loc)[n]   replace_envs
  W 0 t[N] | W n (env t)[n]   rewind(whole | envs)          T t[N]              reload_t_rel
  F                  features_invalidated()                 M 0 | M n env[n]    mark(whole | envs) -> serial
  Q e s              mark_alive(e, s)                       X e / Z             mark_kill(e) / mark_kill_all()
  U e s t max        sdc_rewind_envs' three questions about one row: -> 6 dead, 7 before the mark, 8 overrun (and the mark killed), 0 fine
  N s                next_serial(s)
Every output line: result | rel_hint steps_to_terminal n_feat n_last_done | t_rel[N] | feat[N] | cfg[N] | loc[N] | done[N] | alive[N]"""
import random
import subprocess

import pytest

from dc_rl_amd import _lib as L

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "sdc_mirror.hpp"
static int N = 0;
static bool ints(std::vector<int>& v, const size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; i++)
    if (std::scanf("%d", &v[i]) != 1) return false;
  return true;
}
int main() {
  SdcHostMirror M;
  std::vector<int> serial_of, v, a, b;
  char tag;
  while (std::scanf(" %c", &tag) == 1) {
    int res = 0, n = 0;
    if (tag == 'I') {
      if (!ints(v, 3)) return 2;
      N = v[0];
      M = SdcHostMirror(N, v[1], v[2] != 0);
      serial_of.assign((size_t)N, 0);
    } else if (tag == 'C' || tag == 'L') {
      if (!ints(v, (size_t)N)) return 2;
      if (tag == 'C') M.set_cfg_ids(v.data());
      else M.set_loc_ids(v.data());
    } else if (tag == 'G') {
      if (!ints(v, 3 * (size_t)N)) return 2;
      M.set_cfg_ids(v.data() + 1, 3);
      M.set_loc_ids(v.data() + 2, 3);
    } else if (tag == 'S') {
      if (std::scanf("%d", &n) != 1) return 2;
      res = M.stepped(n);
    } else if (tag == 'E') {
      M.finished_envs_reset();
    } else if (tag == 'R') {
      if (std::scanf("%d", &n) != 1 || (n && !ints(v, (size_t)N))) return 2;
      std::vector<unsigned char> mask(v.begin(), v.end());
      M.reset(n ? mask.data() : nullptr);
    } else if (tag == 'K') {
      if (std::scanf("%d", &n) != 1 || !ints(v, 2 * (size_t)n)) return 2;
      a.clear(), b.clear();
      for (int k = 0; k < n; k++) a.push_back(v[2 * k]), b.push_back(v[2 * k + 1]);
      M.copy_envs(a.data(), b.data(), n);
    } else if (tag == 'P') {
      if (std::scanf("%d", &n) != 1 || !ints(v, 5 * (size_t)n)) return 2;
      std::vector<SdcEnvFacts> f;
      for (int k = 0; k < n; k++) f.push_back({v[5 * k], v[5 * k + 1], v[5 * k + 2] != 0, v[5 * k + 3], v[5 * k + 4]});
      M.replace_envs(f.data(), f.size());
    } else if (tag == 'W') {
      if (std::scanf("%d", &n) != 1) return 2;
      if (n == 0) {
        if (!ints(v, (size_t)N)) return 2;
        M.rewind(nullptr, N, v.data());
      } else {      // (the steps as a column of rows, like a manifest's)
        if (!ints(v, 2 * (size_t)n)) return 2;
        a.clear();
        for (int k = 0; k < n; k++) a.push_back(v[2 * k]);
        M.rewind(a.data(), n, v.data() + 1, 2);
      }
    } else if (tag == 'T') {
      if (!ints(v, (size_t)N)) return 2;
      M.reload_t_rel(v.data());
    } else if (tag == 'F') {
      M.features_invalidated();
    } else if (tag == 'M') {
      if (std::scanf("%d", &n) != 1 || !ints(v, (size_t)n)) return 2;
      res = M.mark(n ? v.data() : nullptr, n);
      for (int k = 0; k < (n ? n : N); k++) serial_of[(size_t)(n ? v[k] : k)] = res;
    } else if (tag == 'Q') {
      if (!ints(v, 2)) return 2;
      res = M.mark_alive(v[0], v[1]);
    } else if (tag == 'X') {
      if (!ints(v, 1)) return 2;
      M.mark_kill(v[0]);
    } else if (tag == 'Z') {
      M.mark_kill_all();
    } else if (tag == 'U') {
      if (!ints(v, 4)) return 2;
      if (!M.mark_alive(v[0], v[1])) res = 6;
      else if (M.steps_since(v[0], v[2]) < 0) res = 7;
      else if (M.steps_since(v[0], v[2]) > v[3]) {
        res = 8;
        M.mark_kill(v[0]);
      }
    } else if (tag == 'N') {
      if (!ints(v, 1)) return 2;
      res = SdcHostMirror::next_serial(v[0]);
    } else {
      return 3;
    }
    std::printf("%d | %d %d %d %d |", res, M.rel_hint(), M.steps_to_terminal(), M.n_feat(), M.n_last_done());
    for (int e = 0; e < N; e++) std::printf(" %d", M.t_rel(e));
    std::printf(" |");
    for (int e = 0; e < N; e++) std::printf(" %d", (int)M.feat(e));
    std::printf(" |");
    for (int e = 0; e < N; e++) std::printf(" %d", M.cfg(e));
    std::printf(" |");
    for (int e = 0; e < N; e++) std::printf(" %d", M.loc(e));
    std::printf(" |");
    for (int e = 0; e < N; e++) std::printf(" %d", M.n_last_done() > 0 ? (int)M.last_done()[e] : 0);
    std::printf(" |");
    for (int e = 0; e < N; e++) std::printf(" %d", (int)M.mark_alive(e, serial_of[(size_t)e]));
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """the driver built by g++ alone (no HIP on the include path): plain, and with the address and undefined-behaviour sanitizers"""
    d = tmp_path_factory.mktemp("mirror")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + L.CSRC, str(src)]
    plain, san = str(d / "driver"), str(d / "driver_san")
    subprocess.run(base + ["-O1", "-o", plain], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san], check=True)
    return plain, san


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    return got


@pytest.fixture(scope="module", params=[0, 1], ids=["plain", "sanitized"])
def ask(drivers, request):
    """operation lines -> per line a dict of the printed state; every hand-written case runs on both builds of the driver"""
    def parse(ln):
        p = [[int(x) for x in part.split()] for part in ln.split("|")]
        return dict(res=p[0][0], rel_hint=p[1][0], left=p[1][1], n_feat=p[1][2], n_done=p[1][3], t=p[2], feat=p[3], cfg=p[4], loc=p[5],
                    done=p[6], alive=p[7])
    return lambda lines: [parse(ln) for ln in _run(drivers[request.param], lines)]


def row(*xs):
    return " ".join(str(int(x)) for x in xs)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
class Model:
    """Every env's facts as plain lists, updated env by env; what the batch is told as a whole is worked out from them when asked."""

    def __init__(self, n, T, has_feat):
        self.n, self.T, self.has_feat = n, T, has_feat
        self.step = [T] * n          # every env finished
        self.rows = [False] * n      # has feature rows
        self.cfg = self.loc = None   # unassigned
        self.finished = []           # envs that finished in the last stepping call
        self.serial = [0] * n        # the env's live mark (0: none)
        self.asked = [0] * n         # the serial of the last mark asked for, per env
        self.last_serial = 0
        # A kept oddity, not a rule of its own: until the first operation that works the derived values out (a reset, a replacement,
        # a rewind, a reload) a fresh batch is told rel_hint -1, although its envs all stand at step T
        self.derived = False

    def rel_hint(self):
        return self.step[0] if self.derived and len(set(self.step)) == 1 else -1

    def left(self):
        return self.T - max(self.step)

    def _begin(self, e):
        self.step[e] = 0
        self.rows[e] = self.rows[e] or self.has_feat
        self.serial[e] = 0

    def _replace(self, e, t, rows, cfg, loc):
        self.step[e], self.rows[e], self.serial[e] = t, bool(rows) and self.has_feat, 0
        if self.cfg is not None:
            self.cfg[e] = cfg
        if self.loc is not None:
            self.loc[e] = loc

    def apply(self, op):
        """-> the result the driver prints for the line"""
        tag, a = op[0], op[1:]
        res = 0
        if tag == "C":
            self.cfg = list(a)
        elif tag == "L":
            self.loc = list(a)
        elif tag == "G":
            self.cfg, self.loc = list(a[1::3]), list(a[2::3])
        elif tag == "S":
            self.step = [t + a[0] for t in self.step]
            self.finished = [e for e in range(self.n) if self.step[e] >= self.T] if self.left() == 0 else []
            res = int(bool(self.finished))
        elif tag == "E":
            for e in range(self.n):
                if self.step[e] >= self.T:
                    self._begin(e)
            self.derived = True
        elif tag == "R":
            for e in range(self.n):
                if a[0] == 0 or a[1 + e]:
                    self._begin(e)
            self.derived = True
        elif tag == "K":
            was = (list(self.step), list(self.rows), self.cfg and list(self.cfg), self.loc and list(self.loc))
            for s, d in zip(a[1::2], a[2::2]):
                self._replace(d, was[0][s], was[1][s], was[2][s] if was[2] else 0, was[3][s] if was[3] else 0)
            self.derived = True
        elif tag == "P":
            for k in range(a[0]):
                self._replace(*a[1 + 5 * k:6 + 5 * k])
            self.derived = True
        elif tag == "W":
            pairs = enumerate(a[1:]) if a[0] == 0 else zip(a[1::2], a[2::2])
            for e, t in pairs:
                self.step[e] = t
            self.derived = True
        elif tag == "T":
            self.step = list(a)
            self.derived = True
        elif tag == "F":
            self.rows = [False] * self.n
        elif tag == "M":
            self.last_serial = res = 1 if self.last_serial == 2 ** 31 - 1 else self.last_serial + 1
            for e in (range(self.n) if a[0] == 0 else a[1:]):
                self.serial[e] = self.asked[e] = res
        elif tag == "Q":
            res = int(a[1] != 0 and self.serial[a[0]] == a[1])
        elif tag == "X":
            self.serial[a[0]] = 0
        elif tag == "Z":
            self.serial = [0] * self.n
        elif tag == "U":
            e, s, then, most = a
            if s == 0 or self.serial[e] != s:
                res = 6
            elif self.step[e] < then:
                res = 7
            elif self.step[e] - then > most:
                res, self.serial[e] = 8, 0
        else:
            raise KeyError(tag)
        return res

    def line(self, res):
        done = [int(e in self.finished) for e in range(self.n)]
        zeros = [0] * self.n
        alive = [int(self.serial[e] != 0 and self.serial[e] == self.asked[e]) for e in range(self.n)]
        parts = [[res], [self.rel_hint(), self.left(), sum(self.rows), len(self.finished)], self.step, [int(r) for r in self.rows],
                 self.cfg or zeros, self.loc or zeros, done, alive]
        return " | ".join(row(*p) for p in parts)


def random_ops(rng, n, T, count):
    """-> (lines, expected lines): operations a caller of the library could issue in this state (steps stay inside the episode, a src is
    no dst, a rewind follows three passed questions), weighted so that episodes end, marks are overrun and lock-step comes and goes"""
    m = Model(n, T, rng.random() < 0.8)
    ops = [("I", n, T, int(m.has_feat))]
    want = [m.line(0)]
    marks = {}      # env -> (serial, its step then, max_steps)
    envs = lambda: rng.sample(range(n), rng.randint(1, n))
    while len(ops) < count:
        kind = rng.choices("SRKPWTFMQXZCLGU", weights=[30, 8, 6, 5, 8, 2, 2, 8, 4, 2, 1, 2, 2, 1, 6])[0]
        new = []
        if kind == "S":
            if m.left() < 1:
                kind = "R"
            else:
                k = m.left() if rng.random() < 0.4 else rng.randint(1, m.left())
                new.append(("S", k))
                if k == m.left() and rng.random() < 0.7:
                    new.append(("E",))
        if kind == "R":
            pick = rng.random()
            if pick < 0.35:
                new.append(("R", 0))
            else:      # the finished envs, or any
                mask = [int(t >= T) for t in m.step] if pick < 0.7 and max(m.step) >= T else [int(rng.random() < 0.5) for _ in range(n)]
                new.append(("R", 1, *mask))
        elif kind == "K" and n > 1:
            if rng.random() < 0.3:      # every env from one src
                s = rng.randrange(n)
                pairs = [(s, d) for d in range(n) if d != s]
            else:
                es = envs() if n > 2 else [0, 1]
                cut = rng.randint(1, max(1, len(es) - 1))
                pairs = [(rng.choice(es[:cut]), d) for d in es[cut:]]
            if pairs:
                new.append(("K", len(pairs), *[x for p in pairs for x in p]))
        elif kind == "P":
            es = envs()
            same = rng.random() < 0.3 and rng.randint(0, T)
            new.append(("P", len(es), *[x for e in es for x in (e, same or rng.randint(0, T), rng.randint(0, 1), rng.randint(0, 2), rng.randint(0, 2))]))
        elif kind == "W" and marks:
            es = list(range(n)) if rng.random() < 0.4 and len(marks) == n else rng.sample(sorted(marks), rng.randint(1, len(marks)))
            new = [("U", e, *marks[e]) for e in es]
            fine = all(m.serial[e] == marks[e][0] and 0 <= m.step[e] - marks[e][1] <= marks[e][2] for e in es)
            if fine:
                new.append(("W", 0, *[marks[e][1] for e in es]) if len(es) == n and es == sorted(es) else
                           ("W", len(es), *[x for e in es for x in (e, marks[e][1])]))
        elif kind == "T":
            new.append(("T", *[rng.randint(0, T) for _ in range(n)]))
        elif kind in "FZ":
            new.append((kind,))
        elif kind == "M":
            es = None if rng.random() < 0.5 else envs()
            new.append(("M", 0) if es is None else ("M", len(es), *es))
        elif kind == "Q":
            e = rng.randrange(n)
            new.append(("Q", e, rng.choice([0, m.asked[e], m.last_serial, max(0, m.last_serial - 1), 12345])))
        elif kind == "X":
            new.append(("X", rng.randrange(n)))
        elif kind in "CL":
            new.append((kind, *[rng.randint(0, 2) for _ in range(n)]))
        elif kind == "G":
            new.append(("G", *[x for _ in range(n) for x in (77, rng.randint(0, 2), rng.randint(0, 2))]))
        elif kind == "U" and marks:
            e = rng.choice(sorted(marks))
            new.append(("U", e, *marks[e]))
        for op in new:
            ops.append(op)
            want.append(m.line(m.apply(op)))
            if op[0] == "M":      # (what a caller keeps of a mark: its manifest)
                for e in (range(n) if op[1] == 0 else op[2:]):
                    marks[e] = (m.last_serial, m.step[e], rng.randint(1, 4))
    return [(op[0] + " " + row(*op[1:])).strip() for op in ops], want


SEQUENCES = [(n, T, 1000 * n + T) for n in (1, 2, 5, 64) for T in (3, 5, 8)]


@pytest.fixture(scope="module")
def sequences():
    return [random_ops(random.Random(seed), n, T, 3000 if n < 64 else 1500) for n, T, seed in SEQUENCES]


def test_random_sequences_against_the_model(drivers, sequences):
    seen = set()
    for (n, T, _), (lines, want) in zip(SEQUENCES, sequences):
        got = _run(drivers[0], lines)
        bad = [(i, lines[i], got[i], want[i]) for i in range(len(lines)) if got[i].split() != want[i].split()]
        assert not bad, (n, T, len(bad), bad[0], lines[max(0, bad[0][0] - 5):bad[0][0]])
        seen |= {(ln.split()[0], g.split()[0]) for ln, g in zip(lines, got)}
    # the sequences reached what they were built to reach: episode ends with and without a reset, every answer about a mark
    assert {("S", "1"), ("S", "0"), ("E", "0"), ("U", "0"), ("U", "6"), ("U", "7"), ("U", "8"), ("W", "0"), ("Q", "1"), ("Q", "0")} <= seen


def test_the_sanitizer_build_agrees_and_finds_nothing(drivers, sequences):
    for lines, _ in sequences:
        assert _run(drivers[1], lines) == _run(drivers[0], lines)


# ---- cases written out by hand -----------------------------------------------------------------------------------------------------------
def test_a_fresh_mirror_is_finished_until_a_reset(ask):
    fresh, assigned, reset = ask(["I 4 6 1", "C 1 0 1 0", "R 0"])
    assert fresh["t"] == [6] * 4 and fresh["left"] == 0 and fresh["rel_hint"] == -1      # nothing may step, no kernel is told a step
    assert fresh["n_feat"] == 0 and fresh["cfg"] == fresh["loc"] == [0] * 4 and fresh["n_done"] == 0 and fresh["alive"] == [0] * 4
    assert assigned["cfg"] == [1, 0, 1, 0] and assigned["loc"] == [0] * 4 and assigned["rel_hint"] == -1 and assigned["left"] == 0
    assert reset["t"] == [0] * 4 and reset["left"] == 6 and reset["rel_hint"] == 0 and reset["n_feat"] == 4 and reset["feat"] == [1] * 4
    # an engine without feature rows never has any
    assert ask(["I 2 6 0", "R 0", "P 1 0 3 1 0 0"])[-1]["n_feat"] == 0


def test_lock_step_is_lost_by_a_masked_reset_and_regained(ask):
    out = ask(["I 4 8 1", "R 0", "S 3", "R 1 0 1 0 0", "S 2", "R 1 1 0 1 1"])
    assert [o["rel_hint"] for o in out] == [-1, 0, 3, -1, -1, -1]
    assert out[3]["t"] == [3, 0, 3, 3] and out[3]["left"] == 5
    assert out[5]["t"] == [0, 2, 0, 0] and out[5]["left"] == 6      # (resetting the OTHER envs to step 0 does not meet env 1 at step 2)
    # ... regained when the rest is reset to the same step
    out = ask(["I 3 8 1", "R 0", "S 2", "R 1 1 0 0", "R 1 0 1 1"])
    assert [o["rel_hint"] for o in out] == [-1, 0, 2, -1, 0] and out[-1]["left"] == 8


def test_clones_break_and_restore_lock_step(ask):
    out = ask(["I 4 8 1", "C 0 1 2 0", "L 2 1 0 0", "R 0", "S 2", "R 1 0 0 0 1", "S 1", "K 1 3 0", "K 3 3 0 3 1 3 2"])
    assert out[6]["t"] == [3, 3, 3, 1] and out[6]["rel_hint"] == -1
    assert out[7]["t"] == [1, 3, 3, 1] and out[7]["rel_hint"] == -1 and out[7]["left"] == 5      # a clone from an env at another step
    assert out[7]["cfg"] == [0, 1, 2, 0] and out[7]["loc"] == [0, 1, 0, 0]                       # ... takes its config and location
    assert out[8]["t"] == [1] * 4 and out[8]["rel_hint"] == 1 and out[8]["left"] == 7            # every env from one src
    assert out[8]["cfg"] == [0] * 4 and out[8]["loc"] == [0] * 4
    # unassigned ids stay unassigned through a replacement
    assert ask(["I 2 8 1", "R 0", "P 1 1 4 1 2 2"])[-1]["cfg"] == [0, 0]


def test_a_whole_batch_rewind_keeps_rel_hint(ask):
    out = ask(["I 3 8 1", "R 0", "S 2", "M 0", "S 3", "W 0 2 2 2", "S 1", "W 2 0 2 2 2"])
    assert [o["rel_hint"] for o in out] == [-1, 0, 2, 2, 5, 2, 3, -1]
    assert out[5]["left"] == 6 and out[5]["alive"] == [1, 1, 1] and out[7]["t"] == [2, 3, 2] and out[7]["left"] == 5
    assert out[7]["alive"] == [1, 1, 1] and out[7]["n_feat"] == 3      # the mark survives, the feature rows are the episode's


def test_what_kills_a_mark(ask):
    start = ["I 6 4 1", "R 0", "S 1", "M 0"]
    out = ask(start + ["W 0 1 1 1 1 1 1", "R 1 1 0 0 0 0 0", "K 1 5 1", "P 1 2 1 1 0 0", "M 1 3", "Q 3 1", "Q 3 2", "S 3", "E"])
    assert out[3]["res"] == 1 and out[3]["alive"] == [1] * 6
    assert out[4]["alive"] == [1] * 6                                   # a rewind
    assert out[5]["alive"] == [0, 1, 1, 1, 1, 1]                        # a reset
    assert out[6]["alive"] == [0, 0, 1, 1, 1, 1]                        # a clone INTO the env (its src keeps its mark)
    assert out[7]["alive"] == [0, 0, 0, 1, 1, 1]                        # a restore into it
    assert out[8]["res"] == 2 and out[8]["alive"] == [0, 0, 0, 1, 1, 1]     # a later mark: alive, but it is the later one
    assert out[9]["res"] == 0 and out[10]["res"] == 1
    assert out[11]["res"] == 1 and out[11]["done"] == [0, 1, 1, 1, 1, 1] and out[11]["alive"] == [0, 0, 0, 1, 1, 1]     # an episode's end alone: no
    assert out[12]["alive"] == [0] * 6 and out[12]["t"] == [3, 0, 0, 0, 0, 0]      # the auto-reset of the finished envs
    assert ask(start + ["Z"])[-1]["alive"] == [0] * 6
    assert ask(start + ["X 4"])[-1]["alive"] == [1, 1, 1, 1, 0, 1]
    # an overrun: more steps since the mark than its rows reach -- dead for good, a rewind back inside its reach included
    out = ask(["I 2 8 1", "R 0", "M 0", "S 3", "U 0 1 0 3", "U 1 1 0 2", "U 1 1 0 2", "W 1 1 0", "U 1 1 0 2", "U 0 1 4 3"])
    assert [o["res"] for o in out[4:]] == [0, 8, 6, 0, 6, 7]
    assert out[5]["alive"] == [1, 0]


def test_operations_are_self_contained(ask):
    # the finished envs' reset need not follow its stepped() directly: whatever ran in between, it finds the envs at the episode's end
    out = ask(["I 3 4 1", "R 0", "S 1", "R 1 0 0 1", "S 3", "M 0", "Q 0 1", "E", "S 1"])
    assert out[4]["res"] == 1 and out[4]["t"] == [4, 4, 3] and out[7]["t"] == [0, 0, 3] and out[7]["left"] == 1 and out[7]["alive"] == [0, 0, 1]
    assert out[8]["t"] == [1, 1, 4] and out[8]["done"] == [0, 0, 1]
    out = ask(["I 2 6 1", "R 0", "S 2", "E", "S 1"])      # ... and with none there it changes nothing
    assert out[3]["t"] == [2, 2] and out[3]["rel_hint"] == 2 and out[3]["left"] == 4 and out[4]["t"] == [3, 3]
    # a mirror of no envs (default-constructed) takes every operation that names no env
    out = ask(["R 0", "E", "F", "Z", "M 0", "K 0", "P 0", "T", "S 0"])
    assert all(o["t"] == [] and o["rel_hint"] == -1 and o["left"] == 0 and o["n_feat"] == 0 for o in out)


def test_asking_about_a_mark_before_any_was_taken(ask):
    out = ask(["I 3 5 1", "Q 2 1", "Q 0 0", "X 1", "Z", "U 1 1 0 4", "R 0", "Q 2 1", "M 1 1", "Q 2 1", "Q 1 1", "Q 1 0"])
    assert [o["res"] for o in out] == [0, 0, 0, 0, 0, 6, 0, 0, 1, 0, 1, 0]


def test_the_serial_wraps_past_zero(ask):
    out = ask(["I 1 5 1", "N 0", "N 1", f"N {2 ** 31 - 2}", f"N {2 ** 31 - 1}", "M 0", "M 0"])
    assert [o["res"] for o in out[1:]] == [1, 2, 2 ** 31 - 1, 1, 1, 2]


def test_reads_between_a_step_and_the_next_fold_are_folded(ask):
    out = ask(["I 3 9 1", "R 0", "S 2", "R 1 0 1 0", "S 1", "S 3", "M 1 2", "U 2 1 3 4", "U 2 1 7 4", "K 1 0 1", "S 2", "T 1 2 3", "S 1", "S 5"])
    assert out[4]["t"] == [3, 1, 3] and out[5]["t"] == [6, 4, 6] and out[5]["left"] == 3      # steps launched, nothing folded: reads are exact
    assert out[7]["res"] == 0 and out[8]["res"] == 7                                         # steps since a mark, likewise
    assert out[9]["t"] == [6, 6, 6] and out[9]["rel_hint"] == 6                               # a clone copies the src's step of NOW
    assert out[10]["t"] == [8, 8, 8] and out[10]["rel_hint"] == 8 and out[10]["left"] == 1
    assert out[11]["t"] == [1, 2, 3] and out[11]["left"] == 6                                 # a reload drops the pending steps with the old values
    assert out[12]["t"] == [2, 3, 4] and out[13]["t"] == [7, 8, 9] and out[13]["res"] == 1 and out[13]["done"] == [0, 0, 1]
    assert out[13]["n_done"] == 1 and out[13]["left"] == 0 and out[13]["rel_hint"] == -1
    # last_done names the finished envs of the LAST stepping call only
    out = ask(["I 2 6 1", "R 0", "S 3", "R 1 0 1", "S 3", "R 1 1 0", "S 1"])
    assert out[4]["done"] == [1, 0] and out[5]["done"] == [1, 0] and out[5]["n_done"] == 1 and out[6]["n_done"] == 0 and out[6]["done"] == [0, 0]

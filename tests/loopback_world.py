"""Test-only sequential loopback "world": the ranks of a sharded plan run strictly ONE AFTER ANOTHER in one process (on one
GPU), and only the collectives are replaced.  No threads, no concurrent kernels of different ranks: a tile's two workgroups and
the member fan stay co-resident, nothing waits on a partner that is not running - so, unlike ``tests/test_distributed_gpu.py``
(several processes on one GPU, tile split off), a rank here launches the geometry it launches when it owns a GPU.

A collective cannot complete while only one rank has run, so the world REPLAYS.  A pass runs every rank's function from the same
starting state (the caller's ``reset(rank)`` restores what a separate process would own); a rank's collectives are numbered in
call order.

* every contribution to collective k is known from an earlier pass: the rank gets the true result (element-wise MAX for the
  reduce, the list of parts for the all-gather) - and its contribution must be BIT-IDENTICAL to the one recorded (the programs
  are deterministic; for kernels this is a determinism check across fresh launches);
* the first collective of a rank that is not fully known yet: the contribution is recorded and the rank gets a placeholder (its
  own words for the reduce, zeros for the other parts of a gather).  From there to the end of that pass the rank is TAINTED:
  nothing it contributes is recorded, its result is discarded.

Passes repeat until every rank finishes one untainted.  Every pass but the last completes exactly one collective, so a run of
C collectives takes C + 1 passes; a pass that completes none (ranks that disagree on the number of collectives) is an error,
never another round.  ``world.log[(pass, rank, k)]`` keeps what every rank contributed and got back, for the post-mortem.

Never used by the product."""

import numpy as np


class LoopbackError(AssertionError):
    pass


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class _RankComm(object):
    """What ONE rank sees of the world during ONE pass."""

    def __init__(self, world, rank, pass_no):
        self._w, self.rank, self.world, self.pass_no = world, int(rank), world.world, pass_no
        self.calls = 0              # collectives issued so far in this pass
        self.tainted = False

    # ------------------------------------------------------------------ the two collectives, on NumPy arrays
    def _collective(self, kind, mine):
        w, k = self._w, self.calls
        self.calls += 1
        mine = np.array(mine)                       # (a copy: the caller may reuse its buffer)
        entry = dict(kind=kind, contribution=mine, tainted=self.tainted, known=False)
        w.log[(self.pass_no, self.rank, k)] = entry
        if self.tainted:
            return None
        if k > len(w.collectives):
            raise LoopbackError("rank %d reached collective %d untainted while collective %d is unknown" % (self.rank, k, k - 1))
        if k == len(w.collectives):
            w.collectives.append(dict(kind=kind, parts=[None] * self.world))
        col = w.collectives[k]
        if col["kind"] != kind:
            raise LoopbackError("collective %d is a %s on rank %d and a %s on another rank" % (k, kind, self.rank, col["kind"]))
        have = col["parts"][self.rank]
        if have is not None and not _same_bits(have, mine):
            raise LoopbackError("rank %d: contribution to collective %d (%s) in pass %d is not bit-identical to the one it "
                                "recorded in an earlier pass" % (self.rank, k, kind, self.pass_no))
        if all(p is not None for p in col["parts"]):
            entry["known"] = True
            return col
        col["parts"][self.rank] = mine
        other = next((p for p in col["parts"] if p is not None and (p.shape != mine.shape or p.dtype != mine.dtype)), None)
        if other is not None:
            raise LoopbackError("collective %d (%s): rank %d contributes %s %s, another rank %s %s"
                                % (k, kind, self.rank, mine.dtype, mine.shape, other.dtype, other.shape))
        self.tainted = True
        return None

    def reduce_max(self, words):
        """MAX all-reduce of an integer array; returns the reduced array (a placeholder - the rank's own words - while the
        collective is not fully known)."""
        words = np.asarray(words)
        col = self._collective("reduce", words)
        out = np.array(words) if col is None else np.maximum.reduce(col["parts"])
        self._w.log[(self.pass_no, self.rank, self.calls - 1)]["result"] = out
        return out

    def all_gather(self, part):
        """All-gather of equally shaped arrays; returns the list of ``world`` parts (zeros for the other ranks' while the
        collective is not fully known)."""
        part = np.asarray(part)
        col = self._collective("gather", part)
        if col is None:
            out = [np.array(part) if r == self.rank else np.zeros_like(part) for r in range(self.world)]
        else:
            out = [np.array(p) for p in col["parts"]]
        self._w.log[(self.pass_no, self.rank, self.calls - 1)]["result"] = out
        return out

    # ------------------------------------------------------------------ the two shapes the product uses
    def reduce(self, payload):
        """``reduce(payload)`` of ``NativeStep(..., shard=(rank, world, reduce))`` / ``MPCController._reduce_payload``: int64 MAX
        all-reduce of a (CUDA) tensor in place.  The read-back waits for the launch and the payload kernel in front of it."""
        import torch
        assert payload.dtype == torch.int64 and payload.dim() == 1
        out = self.reduce_max(payload.cpu().numpy())
        payload.copy_(torch.from_numpy(np.ascontiguousarray(out)))

    def install(self, controller):
        """Replace the collectives of an ``MPCController`` INSTANCE: ``_dist``, ``_all_gather`` and ``_agree`` (the MAX all-reduce
        of ``[flag, digest, MASK - digest]``, with the product's own digest source and its refusal).  Everything else - the draw,
        the slice, the launch, the status read, the relaunch protocol, the padding, the refit - stays the controller's."""
        import torch
        comm = self

        def _dist():
            return comm.rank, comm.world

        def _all_gather(mine, world):
            assert world == comm.world
            parts = comm.all_gather(mine.detach().cpu().numpy())
            return [torch.from_numpy(np.ascontiguousarray(p)).to(mine.device) for p in parts]

        def _agree(flag, world):
            assert world == comm.world
            d = controller._rank_digest()
            v = comm.reduce_max(np.array([1 if flag else 0, d, controller.DIGEST_MASK - d], dtype=np.int64))
            if int(v[1]) + int(v[2]) != controller.DIGEST_MASK:
                raise controller._digest_error()
            return bool(int(v[0]))

        controller._dist = _dist
        controller._all_gather = _all_gather
        controller._agree = _agree
        controller._reduce_payload = comm.reduce
        return controller


class LoopbackWorld(object):
    def __init__(self, world, reset=None, max_collectives=32):
        """``reset(rank)``: called before every (pass, rank) - restores everything a separate process would own (generator
        states, counters, the shared context's policies).  ``max_collectives``: the run refuses to go on beyond that many."""
        assert world >= 1
        self.world = int(world)
        self.reset = reset
        self.max_collectives = int(max_collectives)
        self.collectives = []       # k -> dict(kind=, parts=[one array per rank])
        self.log = {}               # (pass, rank, k) -> dict(kind=, contribution=, result=, tainted=, known=)
        self.calls = None           # per rank: collectives of its final (untainted) pass
        self.passes = 0

    def _known(self):
        return sum(1 for c in self.collectives if all(p is not None for p in c["parts"]))

    def result(self, k):
        """The true result of collective ``k`` of the finished run."""
        col = self.collectives[k]
        return np.maximum.reduce(col["parts"]) if col["kind"] == "reduce" else [np.array(p) for p in col["parts"]]

    def run(self, fn):
        """Run ``fn(rank, comm)`` for every rank, pass after pass, until every rank has finished a pass untainted.  Returns the
        list of the ranks' results of that last pass."""
        assert self.passes == 0, "a LoopbackWorld runs one program"
        results = [None] * self.world
        while True:
            self.passes += 1
            known_before = self._known()
            comms = []
            for rank in range(self.world):
                if self.reset is not None:
                    self.reset(rank)
                comm = _RankComm(self, rank, self.passes)
                out = fn(rank, comm)
                results[rank] = None if comm.tainted else out
                comms.append(comm)
            known = self._known()
            if not any(c.tainted for c in comms):
                counts = [c.calls for c in comms]
                if len(set(counts)) != 1 or counts[0] != len(self.collectives) or known != len(self.collectives):
                    raise LoopbackError("the ranks finished with different numbers of collectives: %r (%d known)" % (counts, known))
                if self.passes != known + 1:
                    raise LoopbackError("%d collectives took %d passes, not %d" % (known, self.passes, known + 1))
                self.calls = counts
                return results
            if known != known_before + 1:
                pending = [(k, [r for r, p in enumerate(c["parts"]) if p is None]) for k, c in enumerate(self.collectives)
                           if any(p is None for p in c["parts"])]
                raise LoopbackError("pass %d completed no collective (the ranks disagree on their number or order: collective, "
                                    "ranks that never reached it = %r): not looping further" % (self.passes, pending))
            if known > self.max_collectives:
                raise LoopbackError("more than %d collectives in one run" % self.max_collectives)

"""GPU (-m gpu): MellowWrapper.generate(num_return_sequences=n) sharded over two data-parallel ranks (both on device 0, rendezvous
over gloo, as in tests/test_gpu_dp.py): shards stay whole examples, a shard's rows start at lo * n, and the one gather carries
n rows per example.  The engines run in "f32", where a row does not depend on which examples share its call: every rank must
return exactly the six answers of a single-rank call."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from mellow_amd import synth, MellowWrapper
dist.init_process_group(backend="gloo")
rank, world = dist.get_rank(), dist.get_world_size()
assert world == 2
_calls = []
_ag = dist.all_gather
def _counted(*a, **k):
    _calls.append("all_gather")
    return _ag(*a, **k)
dist.all_gather = _counted
class Tok:
    def encode(self, s): return [0] if s == "<|endoftext|>" else [17 + (sum(s.encode()) * 7919 + i * 104729) % 49000 for i, _ in enumerate(s.split())]
    def encode_plus(self, text, max_length=129, **kw):
        ids = self.encode(text)[:max_length]
        return {"input_ids": torch.tensor([ids + [1] * (max_length - len(ids))]), "attention_mask": torch.tensor([[1] * max_length])}
    def decode(self, ids): return " ".join("<|endoftext|>" if int(i) == 0 else f"t{int(i)}" for i in ids)
sd = synth.make_state_dict(0)
kw = dict(config="v0", model="v0", device=0, use_cuda=True, state_dict=sd, tokenizer=Tok(), max_positions=512, precision="f32")
m = MellowWrapper(data_parallel=True, **kw)
a1, a2, _ = synth.make_batch(3, n_samples=2 * 32000)
examples = [[a1[i], a2[i], f"question number {i} about the two clips"] for i in range(3)]
dist.barrier()
del _calls[:]
got = m.generate(examples=examples, max_len=6, top_p=0.9, temperature=0.7, do_sample=True, seed=7, num_return_sequences=2)
assert _calls == ["all_gather"], _calls
assert len(got) == 3 and all(isinstance(g, list) and len(g) == 2 for g in got), got
alone = MellowWrapper(data_parallel=False, **kw)
want = alone.generate(examples=examples, max_len=6, top_p=0.9, temperature=0.7, do_sample=True, seed=7, num_return_sequences=2)
flat = alone.generate(examples=[examples[i // 2] for i in range(6)], max_len=6, top_p=0.9, temperature=0.7, do_sample=True, seed=7)
assert got == want, (rank, got, want)
assert [a for g in want for a in g] == flat, (rank, want, flat)          # ... which are those of every example given twice
try:                                                                       # n is part of what the ranks agree on
    m.generate(examples=examples, max_len=6, top_p=0.9, temperature=0.7, do_sample=True, seed=7, num_return_sequences=2 + rank)
    raise SystemExit("ranks with different num_return_sequences were accepted")
except ValueError as e:
    assert "different `examples` or sampling arguments" in str(e), e
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_two_ranks_return_the_answers_of_one(tmp_path):
    script = tmp_path / "nseq_dp_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29771", OMP_NUM_THREADS="8", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29771", str(script), ROOT]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.count("ok") == 2

"""torch hands out its side streams round robin from a pool of 32 per device, and tests/test_graph_replay_gpu.py compares
pool-stream handles (a warm-up stream there must not be the stream `torch.cuda.graph` captures on by default), so how many
streams were created before that file decides what it sees.  `neutral_stream_pool()` lets a test module create as many
streams as its code under test needs — `Trainer._capture` and `GraphedForward` make one per capture or wrapper — and leaves
the round robin where the module found it."""
import contextlib

import torch

POOL = 32


@contextlib.contextmanager
def neutral_stream_pool():
    first = torch.cuda.Stream().cuda_stream                    # slot c of the round robin
    try:
        yield
    finally:
        for _ in range(2 * POOL):                              # on to slot c again: the counter then stands one past the start
            if torch.cuda.Stream().cuda_stream == first:
                break
        else:
            raise AssertionError("the stream pool did not come round to its first stream within %d streams" % (2 * POOL))
        for _ in range(POOL - 1):                              # and once round, less that one
            torch.cuda.Stream()

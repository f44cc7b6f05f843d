"""The member lengths and split targets at which the lockstep-batch tests reach every split of the
batched level launch — TEST INFRASTRUCTURE ONLY.

Nothing here restates the plan rule: every value comes from ccj_amd.batch_level_plan (include/ccj.h
ccj_batch_level_plan, the function the launch itself uses).  tests/test_lockstep_plan.py pins, on the
CPU, what each target reaches; tests/test_gpu_lockstep.py folds under the same targets.
"""
from ccj_amd import DEFAULT_SPLIT_TARGET, batch_level_plan

# long and short alternating, the lengths without any 4-D level (n <= 2) beside the longest; all are
# lengths of Turner04 d2 fixtures of tests/golden/hashes.json
LENGTHS = (54, 1, 50, 2, 33, 3, 20)

# resolved split target -> the splits the batched k_level4d launches of a LENGTHS batch take over its
# levels 0 .. 51 (0 = never split; the default target splits every level of so small a batch 8 ways)
TARGET_SPLITS = {0: {1}, 128: {1, 2}, 512: {1, 2, 4, 8}, DEFAULT_SPLIT_TARGET: {8}}


def levels(lengths):
    return max(max(lengths) - 2, 0)


def splits(lengths, target):
    """The set of splits over every level of the batch."""
    return {batch_level_plan(lengths, t, target).split for t in range(levels(lengths))}


def option(target):
    """The ccj_options.split_target value that resolves to `target` (0 means never split: -1)."""
    return -1 if target == 0 else target

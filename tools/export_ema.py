"""Write the moving average of the weights that a run with --ema_decay stored in a checkpoint as a checkpoint of its own, for
inference: its "model" entry IS the average (vacnic_amd.checkpoint.ema_as_model), optimizer state left out.

    python tools/export_ema.py OUT/runlast.pt OUT/runlast_ema.pt
    python utils/test_mmbart_clip_ddp.py --model_dir OUT --model_name runlast_ema --beam_size 5 ...

Every loader of checkpoints reads the result as plain weights, so the stand-alone caption generator decodes with the weights the
trainer validated with (--ema_eval) without a switch of its own.  Host work only: it needs no GPU.  A checkpoint without an
average is an error, never a silent copy of the weights."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
parser.add_argument("src", help="checkpoint written by a trainer run with --ema_decay")
parser.add_argument("dst", help="inference checkpoint to write (model = the average)")


def export(src, dst):
    from vacnic_amd.checkpoint import ema_as_model
    if os.path.abspath(src) == os.path.abspath(dst):
        raise ValueError("export_ema: source and destination are the same file (the training checkpoint would lose its weights)")
    ck = torch.load(src, map_location="cpu", weights_only=False)
    try:
        out = ema_as_model(ck)
    except KeyError as e:
        raise KeyError(f"{src}: {e.args[0]}") from None
    torch.save(out, dst)
    return out


if __name__ == "__main__":
    a = parser.parse_args()
    out = export(a.src, a.dst)
    print(f"{a.dst}: {len(out['model'])} tensors, the average in place of the weights (step {out['meta'].get('step')})")

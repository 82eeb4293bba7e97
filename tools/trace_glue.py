#!/usr/bin/env python3
"""Lists every ATen op one benchmark-shape forward dispatches (the PyTorch "glue" between libispk launches) with the
isp_tts_amd source line that issued it.  TorchDispatchMode, GPU box."""
import collections, os, sys, traceback, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch.utils._python_dispatch import TorchDispatchMode
from isp_tts_amd import synth
from isp_tts_amd.acoustic.model import AcousticModel
from isp_tts_amd.config import AcousticDims
model = AcousticModel.init(AcousticDims().model_config()).eval()
model.load_state_dict(synth.make_state_dict(), strict=True)
model = model.to("cuda")
model.set_compute_dtype(torch.bfloat16)
model.overlap_streams = False
d = {k: v.to("cuda") for k, v in synth.make_inputs(64, 100, 512).items()}
def step():
    with torch.no_grad():
        return model(d["text"], d["text_len"], d["mel"], d["mel_len"], d["pitch"], d["energy"], flow_noise=d["flow_x0"],
                     flow_time=d["flow_t"])
step(); step(); torch.cuda.synchronize()
SKIP = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select", "aten.unsqueeze",
        "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze", "aten.reshape",
        "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh", "aten._reshape_alias", "aten.split",
        "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty")
log = collections.Counter()
class Spy(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if not name.startswith(SKIP):
            where = "?"
            for fr in reversed(traceback.extract_stack()):
                if "isp_tts_amd" in fr.filename and "runtime.py" not in fr.filename and "/bindings/" not in fr.filename:
                    where = f"{fr.filename.split('isp_tts_amd/')[-1]}:{fr.lineno}"
                    break
            else:
                for fr in reversed(traceback.extract_stack()):
                    if "runtime.py" in fr.filename or "/bindings/" in fr.filename:
                        where = f"{fr.filename.split('isp_tts_amd/')[-1]}:{fr.lineno}"
                        break
            log[(where, name)] += 1
        return func(*args, **(kwargs or {}))
with Spy():
    step()
torch.cuda.synchronize()
for (where, name), n in sorted(log.items()):
    print(f"{n:3d}  {name:40s} {where}")
print("total dispatched (non-view) ops:", sum(log.values()))

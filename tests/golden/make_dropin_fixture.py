"""Writes tests/golden/dropin_reference.json: what the reference's UNMODIFIED model.py does on this repo's drop-in `layers`
package, for tests/test_dropin.py, which runs without the reference tree.

    python tests/golden/make_dropin_fixture.py /path/to/contextflow/contextflow/model.py

Recorded: the names model.py's code takes from `layers` (its `from layers import *` and `from layers.rtdl.nn._embeddings
import *`), and for every model its `create_model` builds here - the mnist / cifar10 / smap generalists and three specialists -
the state_dict layout (names and shapes in order) and the classes that are not this repo's or torch's."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "dropin_reference.json")

DRIVER = r"""
import json, os, sys, types
import torch.nn as nn
sys.dont_write_bytecode = True                      # the reference tree is read-only

def stub(name, **attrs):                            # third-party / dataset modules that are not on the density path
    m = types.ModuleType(name); m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m

class InputDropout(nn.Module):
    def __init__(self, *a, **k): super().__init__()
    def forward(self, x): return x

stub("datasets"); stub("datasets.ts", InputDropout=InputDropout, load_data_ts=None)
stub("datasets.mnist", load_data=None); stub("datasets.cifar10", load_data=None)
stub("datasets.mtad_dataloader", mtad_entities={})
stub("torchinfo", summary=None); stub("ood_metrics", auroc=None, aupr=None, fpr_at_95_tpr=None)

from contextflow_amd import run
M = run.load(sys.argv[1])
import contextflow_amd as cfa

def code_names(co):
    out = set(co.co_names)
    for c in co.co_consts:
        if isinstance(c, types.CodeType):
            out |= code_names(c)
    return out

used = set()
for v in vars(M).values():
    fn = getattr(v, "__code__", None)
    if fn is not None and getattr(v, "__module__", None) == M.__name__:
        used |= code_names(fn)
    if isinstance(v, type) and v.__module__ == M.__name__:
        for f in vars(v).values():
            if hasattr(f, "__code__"):
                used |= code_names(f.__code__)
names = sorted(n for n in used if n in vars(M) and str(getattr(vars(M)[n], "__module__", "")).startswith("contextflow_amd."))

models = []
for name, generalist, contexts, emb, enc, cf in (("mnist", True, [-1], "onehot", "uniform", False),
                                                 ("cifar10", True, [-1, -1], "onehot", "uniform", False),
                                                 ("smap", True, [55], "onehot", "uniform", False),
                                                 ("cifar10", False, [15, 5], "onehot", "uniform", True),
                                                 ("smap", False, [55], "eye", "uniform", False),
                                                 ("mnist", False, [64], "embed", "probsample", True)):
    preset, data_size, mixtures = cfa.preset_config(name)
    M.c = types.SimpleNamespace(dataset=name)       # create_model reads this module global
    cfg = dict(preset, generalist=generalist, enc_emb=emb, enc_type=enc, contextflow=cf)
    flow = M.create_model(cfg, data_size=data_size, mixtures=mixtures, contexts=contexts)
    foreign = sorted({type(m).__qualname__ for m in flow.modules() if not type(m).__module__.startswith(("contextflow_amd.", "torch."))})
    models.append({"name": name, "generalist": generalist, "contexts": contexts, "enc_emb": emb, "enc_type": enc, "contextflow": cf,
                   "flow_class": type(flow).__module__ + "." + type(flow).__qualname__, "foreign_classes": foreign,
                   "state_dict": [[k, list(v.shape)] for k, v in flow.state_dict().items()]})
print(json.dumps({"layers_names": names, "models": models}))
"""


def main():
    script = os.path.abspath(sys.argv[1])
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", DRIVER, script], cwd=os.path.dirname(script), env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr[-4000:])
    fx = json.loads(r.stdout.strip().splitlines()[-1])
    text = json.dumps(fx, indent=1)
    text = re.sub(r"\[\s+([^\[\]]*?)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text)   # a shape on one line
    text = re.sub(r"\[\s+(\"[^\"]*\"),\s+(\[[^\[\]\n]*\])\s+\]", r"[\1, \2]", text)                    # a [name, shape] pair on one line
    with open(OUT, "w") as f:
        f.write(text + "\n")
    print("%s: %d names, %d models" % (OUT, len(fx["layers_names"]), len(fx["models"])))


if __name__ == "__main__":
    main()

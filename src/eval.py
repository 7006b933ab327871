"""`python src/eval.py model=discrete_diffusion ckpt_path=...` (reference: src/eval.py:8-13, src/tasks/eval_task.py:14-62).
`model.use_ema=true` evaluates the averaged weights a run with native_step=true and native_optim.ema_decay keeps in its checkpoint
(checkpoint["gsdd"]["native_adam"]["ema"]; the model wrapper loads them into the generator when the checkpoint is read, and a
checkpoint without them is an error that names the key)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PROJECT_ROOT", ROOT)
import src  # noqa: E402,F401
from gsdd_amd.hydra_lite import compose  # noqa: E402


def main(argv=None):
    cfg = compose(os.path.join(ROOT, "configs"), "eval.yaml", list(argv if argv is not None else sys.argv[1:]))
    from src.tasks.runner import evaluate
    return evaluate(cfg)


if __name__ == "__main__":
    main()

"""Entry point mirroring the reference's ``scripts/run_metrics_dnn_classif.py`` for the classifier outputs: reads the
``*_y_hat_hard.pt`` files written by ``scripts/evaluate_*_net.py`` (and the labels saved beside them), computes
accuracy / precision / recall / F1 per utterance and prints the reference's METRIC / AVERAGE / CONF. INT. table.
With a second directory, the ``*_scores.pt`` files that ``evaluate_main(score_dir=...)`` wrote there give a second table:
SI-SDR, SI-SIR, SI-SAR of the enhanced speech and the input SI-SDR.
Run from the package root: ``python scripts/run_metrics_dnn_classif.py [eval_out [score_dir]]``."""
import sys
sys.path.append('.')

from avvad.train import metrics_main

confidence = 0.95  # confidence interval (name as in the reference script)
eps = 1e-8

if __name__ == '__main__':
    metrics_main(sys.argv[1] if len(sys.argv) > 1 else "eval_out", confidence=confidence, eps=eps,
                 score_dir=sys.argv[2] if len(sys.argv) > 2 else None)

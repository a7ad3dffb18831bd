"""twtml-logistic: StreamingLogisticRegressionWithSGD over the tweet stream.

The LinearRegression driver (``apps/linear_regression.py``) with MLlib's
third streaming learner: the same source, filter, featurizer, prequential
predict + stats then train per micro-batch, report session, ``--checkpoint``
/ ``--resume``, and engines (``--master local[N]`` the fp64 CPU engine,
``--master rocm...`` the MI355X engine with the logistic row epilogue in its
GD kernels).  It answers "will this tweet pass N retweets":

``--labelThreshold N``  a kept tweet is class 1 when ``retweetCount >= N``
                        (default: the middle of the filter range, 550 at the
                        reference's 100..1000; ``labelThreshold`` in
                        ``reference.conf``)
``--threshold P``       predicted class 1 when the probability exceeds P
                        (default 0.5; ``threshold`` in ``reference.conf``)

``-p`` / ``--stepSize`` keeps the shared ``reference.conf`` default (0.005, the
linear model's); MLlib's own default for this learner is 0.1.

Report: labels and predictions are 0 / 1, so the three numbers of the
twtml-web protocol are sent in percent -- ``mse`` is the misclassification
rate of the batch under the model before it trained on it, the two stdevs
those of the 0 / 1 labels and predictions, all times 100 and rounded.

Checkpoints are MLlib ``LogisticRegressionModel`` directories
(``checkpoint/saveable.py``), which ``twtml-score --model`` scores with.
"""
from __future__ import annotations

import logging
import sys
from typing import List, Optional

from ..models.logistic_regression import LogisticRegressionModel
from .linear_regression import LinearRegressionJob, build_engine, run_driver

__all__ = ["main", "LogisticRegressionJob", "build_logistic_engine"]

log = logging.getLogger("com.giorgioinf.twtml.spark.LogisticRegression")
APP_NAME = "twitter-stream-ml-logistic-regression"


def build_logistic_engine(conf, rank: int, world: int, device: Optional[int] = None, max_rows: int = 0):
    return build_engine(conf, rank, world, device, max_rows, loss="logistic")


class LogisticRegressionJob(LinearRegressionJob):
    """Per-batch logic of the logistic driver: the linear job with 0 / 1
    statistics reported in percent and LogisticRegressionModel checkpoints."""

    def _report(self, raw, res, time_ms: int) -> None:
        n, sy, sy2, sp, sp2, se2 = res["stats"]
        # y, p in {0, 1} -> 100 y, 100 p for the stdevs; the mismatch rate se2 / n in percent
        res = dict(res, stats=[n, 100.0 * sy, 1e4 * sy2, 100.0 * sp, 1e4 * sp2, 100.0 * se2])
        super()._report(raw, res, time_ms)

    def _save_model(self, path, weights, prog) -> None:
        LogisticRegressionModel.save_sparse(path, weights, 0.0, float(self.conf.threshold), prog)


def main(argv: Optional[List[str]] = None) -> int:
    return run_driver(argv, APP_NAME, build_logistic_engine, LogisticRegressionJob,
                      lambda path: LogisticRegressionModel.load(path).weights)


if __name__ == "__main__":
    sys.exit(main())

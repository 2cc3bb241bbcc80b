"""Run logging for the trainers.  With MLflow installed, `MlflowLogger` is the reference's (src/utils/logger.py): same calls,
same keys.  Without it, `CsvLogger` writes the same per-epoch keys to <out_dir>/metrics.csv (one row per log_metrics call,
first column the step) and the parameters to <out_dir>/params.csv; artefacts already lie under out_dir and are not copied."""
import csv
from pathlib import Path
from typing import Any, Dict, Optional


class MlflowLogger:
    def __init__(self, tracking_uri: str, experiment_name: str, run_name: Optional[str] = None) -> None:
        import mlflow
        self._mlflow = mlflow
        mlflow.set_tracking_uri(tracking_uri)
        mlflow.set_experiment(experiment_name)
        self._run_ctx = mlflow.start_run(run_name=run_name)

    def log_params(self, params: Dict[str, Any]) -> None:
        self._mlflow.log_params(params)

    def log_metrics(self, metrics: Dict[str, float], step: Optional[int] = None) -> None:
        self._mlflow.log_metrics(metrics, step=step)

    def log_artifact(self, path: Path) -> None:
        self._mlflow.log_artifact(str(path))

    def end(self) -> None:
        self._mlflow.end_run()


class CsvLogger:
    def __init__(self, out_dir: Path) -> None:
        self.out_dir = Path(out_dir)
        self.out_dir.mkdir(parents=True, exist_ok=True)
        self._keys = None

    def log_params(self, params: Dict[str, Any]) -> None:
        with open(self.out_dir / "params.csv", "w", newline="") as f:
            csv.writer(f).writerows([["param", "value"]] + [[k, v] for k, v in params.items()])

    def log_metrics(self, metrics: Dict[str, float], step: Optional[int] = None) -> None:
        fresh = self._keys is None
        if fresh:
            self._keys = list(metrics)
        with open(self.out_dir / "metrics.csv", "w" if fresh else "a", newline="") as f:
            w = csv.writer(f)
            if fresh:
                w.writerow(["step"] + self._keys)
            w.writerow([step] + [metrics.get(k) for k in self._keys])

    def log_artifact(self, path: Path) -> None:
        pass

    def end(self) -> None:
        pass


def make_logger(tracking_uri: str, experiment_name: str, run_name: Optional[str], out_dir: Path):
    """MlflowLogger when `mlflow` imports, else CsvLogger under out_dir."""
    try:
        import mlflow  # noqa: F401
    except ImportError:
        return CsvLogger(out_dir)
    return MlflowLogger(tracking_uri, experiment_name, run_name)

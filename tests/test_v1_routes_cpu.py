"""The reference's ``/api/v1`` REST surface (``master/_v1_routes.py``) against an in-process master:
the added calls behave as the reference's handlers do (request / response field names from the
proto messages)."""

import json
import os
import tempfile

import pytest
import requests

from determined_amd.common.api import APIException, Session

CFG = {"name": "v1", "hyperparameters": {}, "searcher": {"name": "single", "metric": "loss",
                                                        "smaller_is_better": True, "max_length": {"batches": 1}}}


@pytest.fixture()
def master():
    from determined_amd.master import start_master

    srv = start_master()
    yield srv, Session(f"http://127.0.0.1:{srv.port}")
    srv.stop()
    srv.master.close()


def _ndjson(srv, path, **params):
    r = requests.get(f"http://127.0.0.1:{srv.port}{path}", params=params, timeout=30)
    assert r.status_code == 200, r.text
    return [json.loads(line)["result"] for line in r.text.splitlines() if line.strip()]


def _exp(s, n=1, name="v1", cfg=None):
    eid = s.post("/api/v1/unmanaged/experiments", {"config": dict(cfg or CFG, name=name)})["experiment"]["id"]
    tids = [s.post(f"/api/v1/unmanaged/experiments/{eid}/trials", {"hparams": {"i": i}})["trial_id"] for i in range(n)]
    return eid, tids


def test_users_settings_activity_and_master(master):
    srv, s = master
    assert s.get("/api/v1/auth/user")["user"]["username"] == "determined"
    s.post("/api/v1/users/setting", {"settings": [{"key": "theme", "value": "dark", "storage_path": "ui"}]})
    assert s.get("/api/v1/users/setting")["settings"] == [{"key": "theme", "storage_path": "ui", "value": "dark"}]
    s.post("/api/v1/users/setting/reset")
    assert s.get("/api/v1/users/setting")["settings"] == []
    assert s.get("/api/v1/users/admin/by-username")["user"]["username"] == "admin"
    u = s.post("/api/v1/users", {"username": "ann"})["user"]
    g = s.post("/api/v1/groups", {"name": "g1"})["group"]
    s.patch("/api/v1/users/assignments", {"user_ids": [u["id"]], "add_groups": [g["id"]]})
    found = s.post("/api/v1/groups/search", {"user_id": u["id"]})
    assert [x["group"]["name"] for x in found["groups"]] == ["g1"] and found["groups"][0]["num_members"] == 1
    got = s.request("PUT", f"/api/v1/groups/{g['id']}", body={"name": "g2", "remove_users": [u["id"]]})["group"]
    assert got["name"] == "g2" and got["members"] == []
    s.post("/api/v1/users/activity", {"activity_type": "ACTIVITY_TYPE_GET", "entity_type": "ENTITY_TYPE_PROJECT",
                                      "entity_id": 1})
    assert [p["id"] for p in s.get("/api/v1/user/projects/activity")["projects"]] == [1]
    assert s.get("/api/v1/master/telemetry") == {"enabled": False, "segment_key": ""}
    assert s.post("/api/v1/cleanup_logs")["removed_count"] == 0


def test_roles_by_id(master):
    srv, s = master
    u = s.post("/api/v1/users", {"username": "bob"})["user"]
    g = s.post("/api/v1/groups", {"name": "team"})["group"]
    ws = s.post("/api/v1/workspaces", {"name": "w"})["workspace"]
    roles = s.post("/api/v1/roles/search", {})["roles"]
    assert [r["name"] for r in roles] == ["ClusterAdmin", "WorkspaceAdmin", "WorkspaceCreator", "Viewer", "Editor"]
    assert [r["role_id"] for r in roles] == [1, 2, 3, 4, 5]
    scoped = s.post("/api/v1/roles/search/by-assignability", {"workspace_id": ws["id"]})["roles"]
    assert "ClusterAdmin" not in [r["name"] for r in scoped]
    assert s.post("/api/v1/roles/search/by-ids", {"role_ids": [5]})["roles"][0]["name"] == "Editor"
    s.post("/api/v1/roles/add-assignments", {
        "user_role_assignments": [{"user_id": u["id"], "role_assignment": {"role": {"role_id": 4},
                                                                           "scope_workspace_id": ws["id"]}}],
        "group_role_assignments": [{"group_id": g["id"], "role_assignment": {"role": {"role_id": 5}}}]})
    by_user = s.get(f"/api/v1/roles/search/by-user/{u['id']}")["roles"]
    assert [r["role"]["name"] for r in by_user] == ["Viewer"]
    assert by_user[0]["user_role_assignments"][0]["role_assignment"]["scope_workspace_id"] == ws["id"]
    by_group = s.get(f"/api/v1/roles/search/by-group/{g['id']}")
    assert by_group["assignments"] == [{"role_id": 5, "scope_workspace_ids": [], "scope_cluster": True}]
    on_ws = s.get(f"/api/v1/roles/workspace/{ws['id']}")
    assert [x["username"] for x in on_ws["users_assigned_directly"]] == ["bob"]
    s.post("/api/v1/roles/remove-assignments", {
        "user_role_assignments": [{"user_id": u["id"], "role_assignment": {"role": {"role_id": 4},
                                                                           "scope_workspace_id": ws["id"]}}]})
    assert s.get(f"/api/v1/roles/search/by-user/{u['id']}")["roles"] == []
    summ = s.get("/api/v1/permissions/summary")  # the default user is a cluster admin in auth mode none
    assert summ["roles"][0]["name"] == "ClusterAdmin" and summ["assignments"][0]["scope_cluster"]
    with pytest.raises(APIException):
        s.post("/api/v1/roles/search/by-ids", {"role_ids": [42]})


def test_experiment_calls(master):
    srv, s = master
    e1, (t1,) = _exp(s, name="alpha")
    e2, (t2,) = _exp(s, name="beta")
    s.request("PUT", f"/api/v1/experiments/{e1}/labels/fast")
    s.request("PUT", f"/api/v1/experiments/{e2}/labels/fast")
    assert s.request("PUT", f"/api/v1/experiments/{e2}/labels/big")["labels"] == ["fast", "big"]
    assert s.get("/api/v1/experiment/labels")["labels"] == ["fast", "big"]
    assert s.delete(f"/api/v1/experiments/{e2}/labels/big")["labels"] == ["fast"]
    # bulk actions under the reference's paths, with BulkExperimentFilters
    res = s.post("/api/v1/experiments/archive", {"filters": {"name": "alp"}})["results"]
    assert [r["id"] for r in res] == [e1]
    res = s.post("/api/v1/experiments/unarchive", {"filters": {"labels": ["fast"], "excluded_experiment_ids": [e2]}})
    assert [r["id"] for r in res["results"]] == [e1]
    # retain logs
    s.request("PUT", f"/api/v1/experiments/{e1}/retain_logs", body={"num_days": 3})
    assert s.get(f"/api/v1/trials/{t1}")["trial"]["id"] == t1
    out = s.request("PUT", "/api/v1/experiments/retain_logs", body={"experiment_ids": [e1, e2], "num_days": 7})
    assert [r["error"] for r in out["results"]] == ["", ""]
    s.request("PUT", f"/api/v1/trials/{t2}/retain_logs", body={"num_days": 1})
    rows = srv.master.db.all("SELECT id, log_retention_days FROM trials ORDER BY id")
    assert [r["log_retention_days"] for r in rows] == [7, 1]
    # move
    ws = s.post("/api/v1/workspaces", {"name": "w"})["workspace"]
    proj = s.post(f"/api/v1/workspaces/{ws['id']}/projects", {"name": "p"})["project"]
    s.post("/api/v1/experiments/move", {"experiment_ids": [e2], "destination_project_id": proj["id"]})
    found = s.get("/api/v1/experiments-search", params={"project_id": proj["id"]})
    assert [x["experiment"]["id"] for x in found["experiments"]] == [e2] and found["pagination"]["total"] == 1
    # metrics: reference ReportTrialMetrics body form, then every read
    s.post(f"/api/v1/trials/{t1}/validation_metrics", {"validation_metrics": {
        "trial_id": t1, "trial_run_id": 1, "steps_completed": 5, "metrics": {"avg_metrics": {"loss": 0.5}}}})
    s.post(f"/api/v1/trials/{t1}/metrics", {"group": "training", "metrics": {
        "trial_id": t1, "steps_completed": 5, "metrics": {"avg_metrics": {"loss": 0.7}, "batch_metrics": []}}})
    for steps, loss in ((10, 0.4), (15, 0.3)):
        s.post(f"/api/v1/trials/{t1}/metrics", {"group": "validation", "steps_completed": steps,
                                               "metrics": {"loss": loss}})
    reps = _ndjson(srv, "/api/v1/trials/metrics/validation_metrics", trial_ids=t1)[0]["metrics"]
    assert [r["metrics"]["avg_metrics"]["loss"] for r in reps] == [0.5, 0.4, 0.3]
    assert [r["group"] for r in _ndjson(srv, "/api/v1/trials/metrics/trial_metrics", trial_ids=t1)[0]["metrics"]] \
        == ["validation", "training", "validation", "validation"]
    ts = s.get("/api/v1/trials/time-series", params={"trial_ids": [t1], "metric_names": ["loss"],
                                                     "group": "validation", "max_datapoints": 2})["trials"][0]
    assert [d["batches"] for d in ts["metrics"][0]["data"]] == [5, 15]
    names = _ndjson(srv, "/api/v1/experiments/metrics-stream/metric-names", ids=e1)[0]
    assert names["searcher_metrics"] == ["loss"] and names["validation_metrics"] == ["loss"]
    assert _ndjson(srv, f"/api/v1/experiments/{e1}/metrics-stream/batches", metric_name="loss",
                   group="validation")[0]["batches"] == [5, 10, 15]
    snap = _ndjson(srv, f"/api/v1/experiments/{e1}/metrics-stream/trials-snapshot", metric_name="loss",
                   group="validation", batches_processed=11, batches_margin=2)[0]["trials"]
    assert snap == [{"trial_id": t1, "hparams": {"i": 0}, "metric": 0.4, "batches_processed": 10}]
    r = requests.get(f"http://127.0.0.1:{srv.port}/api/v1/experiments/{e1}/metrics-stream/trials-sample",
                     params={"metric_name": "loss", "group": "validation"}, timeout=30)
    assert r.status_code == 400 and "single-trial" in r.text  # as the reference: no sampling of one trial
    wl = s.get(f"/api/v1/trials/{t1}/workloads", params={"filter": "FILTER_OPTION_VALIDATION"})["workloads"]
    assert [w["validation"]["total_batches"] for w in wl] == [5, 10, 15]
    pv = s.post("/api/v1/preview-hp-search", {"config": dict(CFG, entrypoint="x:y")})["summary"]
    assert pv["trials"] == [{"count": 1, "unit": {"name": "batches", "value": 1}}]


def test_trials_logs_and_profiler(master):
    srv, s = master
    out = s.request("PUT", "/api/v1/experiments/by-external-id/ext-1", body={
        "create_experiment_request": {"config": "name: ext\nsearcher: {name: single, metric: loss, "
                                                "max_length: {batches: 1}}\nhyperparameters: {}\n"}})
    eid = out["experiment"]["id"]
    assert s.request("PUT", "/api/v1/experiments/by-external-id/ext-1",
                     body={"create_experiment_request": {"config": "name: ext"}})["experiment"]["id"] == eid
    tr = s.request("PUT", "/api/v1/trials", body={"create_trial_request": {"experiment_id": eid, "hparams": {"a": 1},
                                                                           "unmanaged": True},
                                                  "external_trial_id": "t-1"})["trial"]
    assert s.get("/api/v1/trials/by-external-id/ext-1/t-1")["trial"]["id"] == tr["id"]
    started = s.post(f"/api/v1/trials/{tr['id']}/start", {"resume": True})
    assert started["trial_run_id"] == 1 and started["steps_completed"] == 0
    assert s.post(f"/api/v1/trials/{tr['id']}/start", {})["trial_run_id"] == 2
    s.post("/api/v1/task/logs", {"task_id": f"trial-{tr['id']}", "logs": [
        {"log": "hello", "rank": 0}, {"log": "world", "rank": 1}, {"log": "hello again", "rank": 1}]})
    logs = _ndjson(srv, f"/api/v1/trials/{tr['id']}/logs")
    assert [x["message"] for x in logs] == ["hello", "world", "hello again"]
    assert [x["message"] for x in _ndjson(srv, f"/api/v1/trials/{tr['id']}/logs", rank_ids=1, limit=1)] == \
        ["hello again"]
    assert [x["message"] for x in _ndjson(srv, f"/api/v1/trials/{tr['id']}/logs", search_text="hello",
                                          order_by="ORDER_BY_DESC")] == ["hello again", "hello"]
    assert s.get(f"/api/v1/trials/{tr['id']}/logs/fields")["rank_ids"] == [0, 1]
    s.post("/api/v1/trials/profiler/metrics", {"batches": [{
        "labels": {"trial_id": tr["id"], "name": "gpu_util", "agent_id": "a0", "metric_type": "PROFILER_METRIC_TYPE_SYSTEM"},
        "values": [0.5, 0.7], "batches": [1, 2], "timestamps": ["2024-01-01T00:00:00Z", "2024-01-01T00:00:01Z"]}]})
    s.post(f"/api/v1/trials/{tr['id']}/metrics", {"group": "profiling_system", "steps_completed": 3,
                                                  "metrics": {"cpu_util": 12.5}})
    labels = _ndjson(srv, f"/api/v1/trials/{tr['id']}/profiler/available_series")[0]["labels"]
    assert sorted(x["name"] for x in labels) == ["cpu_util", "gpu_util"]
    got = _ndjson(srv, f"/api/v1/trials/{tr['id']}/profiler/metrics", **{"labels.name": "gpu_util"})
    assert got[0]["batch"]["values"] == [0.5, 0.7]


def test_agents_allocations_tasks_and_jobs(master):
    srv, s = master
    s.post("/api/v1/agents/register", {"agent_id": "a0", "slots": 2, "host": "127.0.0.1", "gpu": True})
    ag = s.get("/api/v1/agents/a0")["agent"]
    assert sorted(ag["slots"]) == ["0", "1"] and ag["addresses"] == ["127.0.0.1"]
    assert len(s.get("/api/v1/agents/a0/slots")["slots"]) == 2
    assert s.get("/api/v1/agents/a0/slots/1")["slot"]["id"] == "1"
    with pytest.raises(APIException):
        s.get("/api/v1/agents/a0/slots/7")
    tid = s.post("/api/v1/commands", {"command": ["true"], "slots": 1})["task_id"]
    assert s.get(f"/api/v1/commands/{tid}")["command"]["id"] == tid
    with pytest.raises(APIException):
        s.get(f"/api/v1/notebooks/{tid}")  # wrong kind
    assert s.get("/api/v1/tasks/count")["commands"] >= 0
    aid = f"{tid}.1"
    al = s.get(f"/api/v1/allocations/{aid}")["allocation"]
    assert al["task_id"] == tid and not al["ready"]
    s.post(f"/api/v1/allocations/{aid}/ready")
    s.post(f"/api/v1/allocations/{aid}/resources/a0/daemon")
    s.post(f"/api/v1/allocations/{aid}/proxy_address", {"proxy_address": "10.0.0.1"})
    al = s.get(f"/api/v1/allocations/{aid}")["allocation"]
    assert al["ready"] and al["daemon_resources"] == ["a0"] and al["proxy_address"] == "10.0.0.1"
    rz = s.get(f"/api/v1/allocations/{aid}/resources/a0/rendezvous")["rendezvous_info"]
    assert rz == {"addresses": ["127.0.0.1"], "rank": 0, "slots": [1]}
    s.post(f"/api/v1/allocations/{aid}/acceleratorData", {"accelerator_data": {
        "container_id": "c0", "node_name": "n0", "accelerator_type": "rocm", "accelerator_uuids": ["GPU-0"]}})
    acc = s.get(f"/api/v1/tasks/{tid}/acceleratorData")["accelerator_data"]
    assert acc[0]["accelerator_uuids"] == ["GPU-0"]
    got = s.post(f"/api/v1/allocations/{aid}/notify_container_running",
                 {"request_uuid": "r1", "num_peers": 1, "rank": 0, "data": {"x": 1}})
    assert got["data"] == [{"x": 1}]
    s.post(f"/api/v1/allocations/{aid}/signals/pending_preemption")
    assert s.get(f"/api/v1/allocations/{aid}")["allocation"]["preempt"]
    s.post(f"/api/v1/commands/{tid}/set_priority", {"priority": 7})
    assert s.get(f"/api/v1/commands/{tid}")["config"]["priority"] == 7
    # a queued second command: job queue v2 / stats / update
    t2 = s.post("/api/v1/commands", {"command": ["true"], "slots": 2})["task_id"]
    jobs = s.get("/api/v1/job-queues-v2")["jobs"]
    states = {j["full"]["job_id"]: j["full"]["summary"]["state"] for j in jobs}
    assert states[tid] == "STATE_SCHEDULED" and states[t2] == "STATE_QUEUED"
    st = s.get("/api/v1/job-queues/stats")["results"][0]["stats"]
    assert st == {"queued_count": 1, "scheduled_count": 1}
    s.post("/api/v1/job-queues", {"updates": [{"job_id": t2, "priority": 3}]})
    assert s.get(f"/api/v1/commands/{t2}")["config"]["priority"] == 3
    s.post("/api/v1/job-queues", {"updates": [{"job_id": t2, "ahead_of": tid}]})  # takes the anchor's priority
    assert s.get(f"/api/v1/commands/{t2}")["config"]["priority"] == 7
    with pytest.raises(APIException):  # commands cannot change resource pool (experiments only)
        s.post("/api/v1/job-queues", {"updates": [{"job_id": t2, "resource_pool": "default"}]})
    s.post(f"/api/v1/commands/{t2}/kill")
    # generic task with a context directory
    import base64

    gt = s.post("/api/v1/generic-tasks", {"config": "entrypoint: [python, run.py]\nresources: {slots: 0}\n",
                                          "context_directory": [{"path": "run.py", "content":
                                                                 base64.b64encode(b"print(1)").decode()}]})
    assert json.loads(s.get(f"/api/v1/tasks/{gt['task_id']}/config")["config"])["entrypoint"] == ["python", "run.py"]
    import io
    import tarfile

    tgz = base64.b64decode(s.get(f"/api/v1/tasks/{gt['task_id']}/context_directory")["b64_tgz"])
    with tarfile.open(fileobj=io.BytesIO(tgz)) as tf:
        assert tf.extractfile("run.py").read() == b"print(1)"
    nb = s.post("/api/v1/notebooks", {})["task_id"]
    s.request("PUT", f"/api/v1/notebooks/{nb}/report_idle", body={"idle": True})
    assert s.get(f"/api/v1/notebooks/{nb}")["notebook"]["idle"] is True


def test_models_checkpoints_projects_templates_webhooks(master):
    srv, s = master
    with tempfile.TemporaryDirectory() as d:
        cfg = dict(CFG, checkpoint_storage={"type": "shared_fs", "host_path": d})
        eid, (tid,) = _exp(s, cfg=cfg)
        for u in ("aaaa-1", "bbbb-2"):
            os.makedirs(os.path.join(d, u, "sub"))
            for f in ("model.pt", "sub/opt.pt", "meta.json"):
                open(os.path.join(d, u, f), "w").write("x")
            s.post("/api/v1/checkpoints", {"uuid": u, "trial_id": tid, "steps_completed": 1,
                                           "resources": {"model.pt": 1, "sub/opt.pt": 1, "meta.json": 1}})
        md = s.post("/api/v1/checkpoints/aaaa-1/metadata", {"checkpoint": {"metadata": {"k": "v"}}})
        assert md["checkpoint"]["metadata"] == {"k": "v"}
        s.post("/api/v1/checkpoints/rm", {"checkpoint_uuids": ["aaaa-1"], "checkpoint_globs": ["**/*.pt"]})
        ck = s.get("/api/v1/checkpoints/aaaa-1")["checkpoint"]
        assert ck["state"] == "PARTIALLY_DELETED" and sorted(ck["resources"]) == ["meta.json"]
        assert sorted(os.listdir(os.path.join(d, "aaaa-1"))) == ["meta.json", "sub"]
        s.request("DELETE", "/api/v1/checkpoints", body={"checkpoint_uuids": ["bbbb-2"]})
        assert s.get("/api/v1/checkpoints/bbbb-2")["checkpoint"]["state"] == "DELETED"
        assert not os.path.exists(os.path.join(d, "bbbb-2"))
        # models
        s.post("/api/v1/models", {"name": "mdl", "labels": ["x", "y"]})
        s.post("/api/v1/models", {"name": "mdl2", "labels": ["y"]})
        assert s.get("/api/v1/model/labels")["labels"] == ["y", "x"]
        s.post("/api/v1/models/mdl/versions", {"checkpoint_uuid": "aaaa-1"})
        mv = s.get("/api/v1/models/mdl/versions/1")["model_version"]
        assert mv["checkpoint"]["uuid"] == "aaaa-1" and mv["model"]["name"] == "mdl"
        s.post("/api/v1/models/mdl/archive")
        assert s.get("/api/v1/models/mdl")["model"]["archived"] == 1
        s.post("/api/v1/models/mdl/unarchive")
        ws = s.post("/api/v1/workspaces", {"name": "w2"})["workspace"]
        s.post("/api/v1/models/mdl/move", {"destination_workspace_id": ws["id"]})
        assert s.get("/api/v1/models/mdl")["model"]["workspace"] == "w2"
        # projects
        p = s.post(f"/api/v1/workspaces/{ws['id']}/projects", {"name": "proj"})["project"]
        s.post("/api/v1/experiments/move", {"experiment_ids": [eid], "destination_project_id": p["id"]})
        s.post(f"/api/v1/trials/{tid}/metrics", {"group": "validation", "steps_completed": 1, "metrics": {"loss": 2.0}})
        s.post(f"/api/v1/trials/{tid}/metrics", {"group": "validation", "steps_completed": 2, "metrics": {"loss": 1.0}})
        cols = {c["column"]: c for c in s.get(f"/api/v1/projects/{p['id']}/columns")["columns"]}
        assert cols["hp.i"]["location"] == "LOCATION_TYPE_HYPERPARAMETERS"
        assert cols["validation.loss"]["type"] == "COLUMN_TYPE_NUMBER"
        rng = s.get(f"/api/v1/projects/{p['id']}/experiments/metric-ranges")["ranges"]
        assert rng == [{"metrics_name": "validation.loss", "min": 1.0, "max": 2.0}]
        s.post(f"/api/v1/projects/{p['id']}/notes", {"note": {"name": "a", "contents": "hi"}})
        notes = s.request("PUT", f"/api/v1/projects/{p['id']}/notes",
                          body={"notes": [{"name": "b", "contents": "yo"}]})["notes"]
        assert notes == [{"name": "b", "contents": "yo"}]
        ws3 = s.post("/api/v1/workspaces", {"name": "w3"})["workspace"]
        s.post(f"/api/v1/projects/{p['id']}/move", {"destination_workspace_id": ws3["id"]})
        assert s.get(f"/api/v1/experiments/{eid}")["experiment"]["workspace"] == "w3"
        s.post(f"/api/v1/workspaces/{ws3['id']}/pin")
        assert srv.master.db.one("SELECT COUNT(*) AS n FROM workspace_pins")["n"] == 1
        s.post(f"/api/v1/workspaces/{ws3['id']}/unpin")
        assert srv.master.db.one("SELECT COUNT(*) AS n FROM workspace_pins")["n"] == 0
    # templates
    out = s.post("/api/v1/templates/tpl", {"template": {"name": "tpl", "config": "resources: {slots_per_trial: 2}"}})
    assert out["template"]["config"] == {"resources": {"slots_per_trial": 2}}
    with pytest.raises(APIException):
        s.post("/api/v1/templates/tpl", {"template": {"name": "tpl", "config": "{}"}})
    # webhook test against an unreachable endpoint
    wh = s.post("/api/v1/webhooks", {"url": "http://127.0.0.1:9/hook"})["webhook"]
    assert s.post(f"/api/v1/webhooks/{wh['id']}/test")["completed"] is False


def test_continue_experiment_in_place(master):
    srv, s = master
    m = srv.master
    eid = s.post("/api/v1/experiments", {"config": dict(CFG, entrypoint="x:y", max_restarts=0)})["experiment"]["id"]
    with m.lock:
        exp = m.experiments[eid]
        (tr,) = exp.trials.values()
        assert tr.ops  # the single searcher's validate_after
        m._stop_experiment(exp, "CANCELED")  # pending allocation: dropped, trial CANCELED
    assert s.get(f"/api/v1/experiments/{eid}")["experiment"]["state"] == "CANCELED"
    with pytest.raises(APIException):
        s.post("/api/v1/experiments/continue", {"id": 999})
    got = s.post("/api/v1/experiments/continue", {"id": eid, "override_config": "max_restarts: 3\n"})
    assert got["experiment"]["id"] == eid and got["experiment"]["state"] == "ACTIVE"
    row = m.db.one("SELECT config FROM experiments WHERE id=?", [eid])
    assert row["config"]["max_restarts"] == 3
    with m.lock:
        (tr,) = m.experiments[eid].trials.values()
        assert tr.state == "ACTIVE" and tr.ops and tr.close_requested and tr.allocation is not None
    with pytest.raises(APIException):  # not terminal any more
        s.post("/api/v1/experiments/continue", {"id": eid})


def test_sdk_methods_on_the_new_routes(master):
    """Reference SDK methods served by these routes: Experiment.move_to_project /
    delete_tensorboard_files, Trial.get_checkpoints / stream_metrics, Checkpoint.remove_files,
    Model.move_to_workspace / archive, ModelVersion.reload / iter_metrics, Project notes,
    User.link_with_agent, get_model_labels."""
    from determined_amd.experimental import client

    srv, s = master
    client.login(f"http://127.0.0.1:{srv.port}")
    try:
        with tempfile.TemporaryDirectory() as d:
            eid, (tid,) = _exp(s, cfg=dict(CFG, checkpoint_storage={"type": "shared_fs", "host_path": d}))
            for u, steps in (("cccc-1", 1), ("dddd-2", 2)):
                os.makedirs(os.path.join(d, u))
                for f in ("w.pt", "meta.json"):
                    open(os.path.join(d, u, f), "w").write("x")
                s.post("/api/v1/checkpoints", {"uuid": u, "trial_id": tid, "steps_completed": steps,
                                               "resources": {"w.pt": 1, "meta.json": 1}})
            tr = client.get_trial(tid)
            assert [c.uuid for c in tr.get_checkpoints("steps_completed", "desc")] == ["dddd-2", "cccc-1"]
            s.post(f"/api/v1/trials/{tid}/metrics", {"group": "training", "steps_completed": 1, "metrics": {"l": 1}})
            assert len(list(tr.stream_metrics("training"))) == 1
            ck = client.get_checkpoint("cccc-1")
            ck.remove_files([])  # refresh only
            assert ck.state.value == "COMPLETED" and sorted(ck.resources) == ["meta.json", "w.pt"]
            ck.remove_files(["*.pt"])
            assert ck.state.value == "PARTIALLY_DELETED" and sorted(ck.resources) == ["meta.json"]
            ws = client.create_workspace("sdk-w")
            ws.create_project("sdk-p")
            exp = client.get_experiment(eid)
            exp.move_to_project("sdk-w", "sdk-p")
            assert s.get(f"/api/v1/experiments/{eid}")["experiment"]["project"] == "sdk-p"
            exp.delete_tensorboard_files()
            p = ws.get_project("sdk-p")
            p.add_note("a", "1")
            p.add_note("b", "2")
            p.remove_note("a")
            assert p.notes == [{"name": "b", "contents": "2"}]
            mdl = client.create_model("sdk-m", labels=["z"])
            mv = mdl.register_version("dddd-2")
            mv.reload()
            assert mv.checkpoint.uuid == "dddd-2" and list(mv.iter_metrics()) == []
            mdl.move_to_workspace("sdk-w")
            mdl.archive()
            mdl.reload()
            assert mdl._data["workspace"] == "sdk-w" and mdl._data["archived"] == 1
            assert client.get_model_labels() == ["z"]
            u = client.create_user("linked")
            u.link_with_agent(agent_uid=1001, agent_gid=1001, agent_user="svc", agent_group="svc")
            assert client.get_user_by_id(u.user_id)._data["agent_user_group"]["agent_user"] == "svc"
    finally:
        client.logout()


def test_rbac_guards_on_the_reference_routes():
    """In rbac mode: a user sees and controls only tasks it may (view / edit on the owner and
    workspace), allocation lifecycle calls need the task identity (cluster token) or an admin, and
    experiment searches list only viewable experiments."""
    from determined_amd.master import start_master

    srv = start_master(auth="rbac", auth_token="cluster-secret")
    url = f"http://127.0.0.1:{srv.port}"
    try:
        admin = Session(url, token=Session(url).post("/api/v1/auth/login", {"username": "admin"})["token"])
        for name in ("alice", "bob"):
            admin.post("/api/v1/users", {"username": name, "password": "pw"})
        alice = Session(url, token=Session(url).post("/api/v1/auth/login",
                                                     {"username": "alice", "password": "pw"})["token"])
        bob = Session(url, token=Session(url).post("/api/v1/auth/login",
                                                   {"username": "bob", "password": "pw"})["token"])
        tid = alice.post("/api/v1/commands", {"command": ["true"], "slots": 0})["task_id"]
        assert alice.get(f"/api/v1/commands/{tid}")["command"]["id"] == tid
        for call in (lambda: bob.get(f"/api/v1/commands/{tid}"), lambda: bob.post(f"/api/v1/commands/{tid}/kill"),
                     lambda: bob.get(f"/api/v1/tasks/{tid}/context_directory")):
            with pytest.raises(APIException) as ei:
                call()
            assert ei.value.status == 404
        with pytest.raises(APIException) as ei:  # lifecycle calls: task identity only
            alice.post(f"/api/v1/allocations/{tid}.1/ready")
        assert ei.value.status == 403
        Session(url, token="cluster-secret").post(f"/api/v1/allocations/{tid}.1/ready")
        alice.post(f"/api/v1/commands/{tid}/kill")
        # experiments-search filters what the caller may not view
        ws = admin.post("/api/v1/workspaces", {"name": "private"})["workspace"]
        admin.post(f"/api/v1/workspaces/{ws['id']}/projects", {"name": "p"})
        admin.post("/api/v1/unmanaged/experiments", {"config": dict(CFG, name="secret", workspace="private",
                                                                     project="p")})
        names = [x["experiment"]["name"] for x in bob.get("/api/v1/experiments-search")["experiments"]]
        assert "secret" not in names
        assert "secret" in [x["experiment"]["name"] for x in admin.get("/api/v1/experiments-search")["experiments"]]
    finally:
        srv.stop()
        srv.master.close()


def test_trial_logs_follow_ends_with_the_trial_or_the_client(master):
    import threading
    import time as _t

    srv, s = master
    eid, (tid,) = _exp(s)
    s.post("/api/v1/task/logs", {"task_id": f"trial-{tid}", "logs": [{"log": "first", "rank": 0}]})

    def later():
        _t.sleep(1.0)
        s.post("/api/v1/task/logs", {"task_id": f"trial-{tid}", "logs": [{"log": "second", "rank": 0}]})
        _t.sleep(0.5)
        s.post(f"/api/v1/unmanaged/trials/{tid}/close", {"state": "COMPLETED"})

    threading.Thread(target=later, daemon=True).start()
    got = [x["message"] for x in _ndjson(srv, f"/api/v1/trials/{tid}/logs", follow="true")]
    assert got == ["first", "second"]
    # a client that hangs up on a still-running trial does not leave the stream running
    eid2, (tid2,) = _exp(s, name="other")
    base = threading.active_count()
    r = requests.get(f"http://127.0.0.1:{srv.port}/api/v1/trials/{tid2}/logs", params={"follow": "true"},
                     stream=True, timeout=10)
    _t.sleep(0.3)
    r.close()
    deadline = _t.time() + 10
    while threading.active_count() > base and _t.time() < deadline:
        _t.sleep(0.2)
    assert threading.active_count() <= base


def test_det_trial_logs_filters(master, capsys):
    from determined_amd.cli import main

    srv, s = master
    eid, (tid,) = _exp(s)
    s.post("/api/v1/task/logs", {"task_id": f"trial-{tid}", "logs": [
        {"log": "INFO: starting", "rank": 0}, {"log": "WARNING: slow step", "rank": 1},
        {"log": "ERROR: boom", "rank": 1}, {"log": "plain line", "rank": 0}]})
    url = f"http://127.0.0.1:{srv.port}"

    def run(*args):
        main(["-m", url, "trial", "logs", str(tid), *args])
        return capsys.readouterr().out.splitlines()

    assert run() == ["INFO: starting", "WARNING: slow step", "ERROR: boom", "plain line"]
    assert run("--level", "WARNING") == ["WARNING: slow step", "ERROR: boom"]
    assert run("--rank-id", "1", "--tail", "1") == ["ERROR: boom"]
    assert run("--head", "2") == ["INFO: starting", "WARNING: slow step"]
    assert run("--search", "step") == ["WARNING: slow step"]
    main(["-m", url, "experiment", "logs", str(eid), "--tail", "1"])
    assert capsys.readouterr().out.splitlines() == ["plain line"]


def test_allocation_ready_and_waiting_are_state_transitions(master):
    """AllocationReady / AllocationWaiting (reference allocation.go:350-379): ready logs "Service of
    <task> is available", moves the allocation to RUNNING (never backwards) and persists the ready
    bit; waiting moves it to WAITING; a shell task becomes ready from its banner (readiness check)."""
    srv, s = master
    m = srv.master
    s.post("/api/v1/agents/register", {"agent_id": "rdy", "slots": 2, "host": "127.0.0.1"})
    tid = s.post("/api/v1/commands", {"command": ["true"], "slots": 1})["task_id"]
    aid = f"{tid}.1"
    with m.lock:
        m._schedule()
    assert s.get(f"/api/v1/allocations/{aid}")["allocation"]["state"] == "ASSIGNED"
    s.post(f"/api/v1/allocations/{aid}/ready")
    al = s.get(f"/api/v1/allocations/{aid}")["allocation"]
    assert al["ready"] and al["state"] == "RUNNING"
    assert m.db.one("SELECT is_ready, state FROM live_allocations WHERE id=?", [aid]) == {"is_ready": 1,
                                                                                          "state": "RUNNING"}
    logs = [ln["log"] for ln in s.get(f"/api/v1/tasks/{tid}/logs")["logs"]]
    assert f"Service of {tid} is available" in logs
    s.post(f"/api/v1/allocations/{aid}/waiting")
    al = s.get(f"/api/v1/allocations/{aid}")["allocation"]
    assert al["state"] == "WAITING" and al["waiting"]
    s.post(f"/api/v1/allocations/{aid}/ready")  # RUNNING is behind WAITING: the state does not go back
    assert s.get(f"/api/v1/allocations/{aid}")["allocation"]["state"] == "WAITING"
    # readiness check on a service task's log
    with m.lock:
        from determined_amd.master._core import Allocation

        a = Allocation("svc.1", "svc", 0, kind="SHELL")
        a.state = "ASSIGNED"
        m.allocations[a.id] = a
    m.add_logs("svc", [{"log": "starting"}], "svc.1")
    assert not a.ready
    m.add_logs("svc", [{"log": 'shell server ready on port 4242: {"a": 1}'}], "svc.1")
    assert a.ready and a.state == "RUNNING"
    s.post(f"/api/v1/commands/{tid}/kill")


def test_trials_sample_streams_promoted_and_demoted_trials(master):
    """TrialsSample re-ranks every period: a trial that overtakes the top set is promoted (with its
    hparams and every point so far), the one it displaced is demoted, trials already sent get only
    new points, and the stream ends after the experiment reaches a terminal state."""
    srv, s = master
    cfg = dict(CFG, searcher={"name": "random", "metric": "loss", "smaller_is_better": True, "max_trials": 3,
                              "max_length": {"batches": 10}})
    eid, (t1, t2, t3) = _exp(s, 3, name="samp", cfg=cfg)
    for tid, loss in ((t1, 0.5), (t2, 0.4), (t3, 0.9)):
        s.post(f"/api/v1/trials/{tid}/metrics", {"group": "validation", "steps_completed": 5, "metrics": {"loss": loss}})
    r = requests.get(f"http://127.0.0.1:{srv.port}/api/v1/experiments/{eid}/metrics-stream/trials-sample",
                     params={"metric_name": "loss", "group": "validation", "max_trials": 2, "period_seconds": 1},
                     stream=True, timeout=60)
    lines = r.iter_lines()
    first = json.loads(next(lines))["result"]
    assert sorted(first["promoted_trials"]) == sorted([t1, t2]) and first["demoted_trials"] == []
    assert {t["trial"]["trial_id"]: t["trial"].get("hparams") for t in first["trials"]} == {t2: {"i": 1}, t1: {"i": 0}}
    s.post(f"/api/v1/trials/{t3}/metrics", {"group": "validation", "steps_completed": 10, "metrics": {"loss": 0.1}})
    s.post(f"/api/v1/trials/{t2}/metrics", {"group": "validation", "steps_completed": 10, "metrics": {"loss": 0.35}})
    second = json.loads(next(lines))["result"]
    assert second["promoted_trials"] == [t3] and second["demoted_trials"] == [t1]
    got = {t["trial"]["trial_id"]: t for t in second["trials"]}
    assert [d["value"] for d in got[t3]["data"]] == [0.9, 0.1] and got[t3]["trial"]["hparams"] == {"i": 2}
    assert [d["value"] for d in got[t2]["data"]] == [0.35] and "hparams" not in got[t2]["trial"]  # new points only
    s.post(f"/api/v1/experiments/{eid}/kill")
    rest = [json.loads(x)["result"] for x in lines if x.strip()]  # the stream ends by itself
    assert rest and rest[-1]["promoted_trials"] == [] and rest[-1]["demoted_trials"] == []

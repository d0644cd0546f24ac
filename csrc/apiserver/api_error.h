// Internal to apiserver/: the HTTP error the handlers and the JSON patch
// throw, and the Kubernetes Status body it is answered with.
#pragma once

#include <stdexcept>
#include <string>

#include "common/json.h"

namespace xsched::apiserver {

// An HTTP error with a Kubernetes Status body.
struct ApiError : std::runtime_error {
  ApiError(int c, std::string r, const std::string& m) : std::runtime_error(m), code(c), reason(std::move(r)) {}
  int code;
  std::string reason;
};

inline Json status_obj(int code, const std::string& reason, const std::string& message) {
  Json s = Json::object();
  s.set("kind", Json("Status"));
  s.set("apiVersion", Json("v1"));
  s.set("metadata", Json::object());
  s.set("status", Json(code >= 400 ? "Failure" : "Success"));
  s.set("message", Json(message));
  s.set("reason", Json(reason));
  s.set("code", Json(code));
  return s;
}

}  // namespace xsched::apiserver

// A std::unordered_map, std::unordered_set or std::multimap whose entries
// come and go at a high rate (one per scheduled pod): the nodes of released
// entries are parked and handed to the next acquire, so steady state takes
// nothing from the allocator, and a std::string key keeps its buffer.
//
// Three rules, kept here so that no call site has to:
//  * value scrubbed: a parked node's mapped value is cleared (if it has
//    clear()) or assigned mapped_type{}, so it holds no PodPtr, WaitingPodPtr
//    or callable alive. Keys and set elements stay as they are;
//  * capacity kept: clear() is preferred so a parked vector keeps its buffer;
//  * no direct erase: there is no erase() and no mutable access to the
//    container; entries leave through release(), which parks the node.
//
// No locking inside: an instance lives under the mutex that guards the map.
#pragma once

#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

namespace xsched {

template <class Container>
class RecycledMap {
 public:
  using key_type = typename Container::key_type;
  using value_type = typename Container::value_type;
  using iterator = typename Container::iterator;
  using const_iterator = typename Container::const_iterator;
  using node_type = typename Container::node_type;
  static constexpr size_t kDefaultCap = 4096;  // parked nodes, per instance

  explicit RecycledMap(size_t cap = kDefaultCap) : cap_(cap) {}

  // Unique keys: the entry for `key` and whether this call added it. A present
  // entry is returned untouched (the caller decides what to overwrite); an
  // added one has a scrubbed (or value-initialised) mapped value.
  std::pair<iterator, bool> acquire(const key_type& key) {
    static_assert(kUnique, "keys may repeat: acquire(key, mapped)");
    if (spare_.empty()) {
      if constexpr (kSet) return c_.insert(key);
      else return c_.try_emplace(key);
    }
    auto r = c_.insert(take_spare(key));
    if (!r.inserted) spare_.push_back(std::move(r.node));  // `key` was present
    return {r.position, r.inserted};
  }
  // std::multimap: always adds; the new entry's iterator.
  template <class M>
  iterator acquire(const key_type& key, M&& mapped) {
    static_assert(!kUnique, "unique keys: acquire(key), then write the value");
    if (spare_.empty()) return c_.emplace(key, std::forward<M>(mapped));
    node_type nh = take_spare(key);
    nh.mapped() = std::forward<M>(mapped);
    return c_.insert(std::move(nh));
  }

  void release(const_iterator it) { park(c_.extract(it)); }
  // Unique keys only. False if `key` was not present.
  bool release(const key_type& key) {
    static_assert(kUnique, "release(key) needs unique keys: release the iterator");
    auto it = c_.find(key);
    if (it == c_.end()) return false;
    release(it);
    return true;
  }
  void release_all() {
    while (!c_.empty()) release(c_.begin());
  }

  iterator find(const key_type& key) { return c_.find(key); }
  const_iterator find(const key_type& key) const { return c_.find(key); }
  size_t count(const key_type& key) const { return c_.count(key); }
  bool contains(const key_type& key) const { return c_.find(key) != c_.end(); }
  size_t size() const { return c_.size(); }
  bool empty() const { return c_.empty(); }
  iterator begin() { return c_.begin(); }
  iterator end() { return c_.end(); }
  const_iterator begin() const { return c_.begin(); }
  const_iterator end() const { return c_.end(); }
  const Container& container() const { return c_; }
  size_t parked() const { return spare_.size(); }

 private:
  static constexpr bool kSet = std::is_same_v<key_type, value_type>;
  // Inserting a node handle returns an iterator only where keys may repeat.
  static constexpr bool kUnique =
      !std::is_same_v<decltype(std::declval<Container&>().insert(std::declval<node_type>())), iterator>;

  template <class T, class = void>
  struct has_clear : std::false_type {};
  template <class T>
  struct has_clear<T, std::void_t<decltype(std::declval<T&>().clear())>> : std::true_type {};

  // Copy-assigns into the node's old key object: a string reuses its buffer.
  node_type take_spare(const key_type& key) {
    node_type nh = std::move(spare_.back());
    spare_.pop_back();
    if constexpr (kSet) nh.value() = key;
    else nh.key() = key;
    return nh;
  }

  void park(node_type nh) {
    if (spare_.size() >= cap_) return;  // dropped: the node is freed
    if constexpr (!kSet) {
      using Mapped = typename Container::mapped_type;
      if constexpr (has_clear<Mapped>::value) nh.mapped().clear();
      else nh.mapped() = Mapped{};
    }
    spare_.push_back(std::move(nh));
  }

  Container c_;
  std::vector<node_type> spare_;
  size_t cap_;
};

}  // namespace xsched
